// solve_bound.hip -- solve.hip once more in the bounded form: tpl_placement_solve_bound (include/tpl_learn.h states the move bound
// and the bounded form; tpl_placement.h says why this is a unit of its own and where the two forms part).
#define TPL_PLACEMENT_BOUND_UNIT
#include "solve.hip"
