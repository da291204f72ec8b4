// exact_nodes_move.hip -- exact_nodes.hip once more, on the fourteen features: tpl_placement_exact_nodes_move and
// tpl_placement_exact_labels_move (include/tpl_learn.h states the search from a node and the labels; tpl_placement.h says why this
// is a unit of its own).  Both units are of the bounded form.
#define TPL_PLACEMENT_MOVE_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#include "exact_nodes.hip"
