// exact_move.hip -- exact.hip once more, on the fourteen features: tpl_placement_exact_move (include/tpl_learn.h states the exact
// search; tpl_placement.h says why this is a unit of its own).  Both units are of the bounded form.
#define TPL_PLACEMENT_MOVE_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#include "exact.hip"
