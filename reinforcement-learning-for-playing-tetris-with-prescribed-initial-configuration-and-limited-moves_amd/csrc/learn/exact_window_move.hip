// exact_window_move.hip -- exact_window.hip once more, on the fourteen features: tpl_placement_window_prove_move
// (include/tpl_learn.h states the search over a state's window; tpl_placement.h says why this is a unit of its own).  Both units are of
// the bounded form.
#define TPL_PLACEMENT_MOVE_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#include "exact_window.hip"
