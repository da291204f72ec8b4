// beam_move_bound.hip -- beam.hip once more, on the fourteen features and in the bounded form: tpl_placement_beam_move_bound
// (include/tpl_learn.h states the move bound and the bounded form; tpl_placement.h says why this is a unit of its own).
#define TPL_PLACEMENT_MOVE_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#include "beam.hip"
