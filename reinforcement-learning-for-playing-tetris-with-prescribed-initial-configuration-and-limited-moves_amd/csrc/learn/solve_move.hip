// solve_move.hip -- solve.hip once more, on the fourteen features that add landing height and eroded cells to the twelve of the
// board: tpl_placement_solve_move (include/tpl_learn.h states the rule; tpl_placement.h says why this is
// a unit of its own).
#define TPL_PLACEMENT_MOVE_UNIT
#include "solve.hip"
