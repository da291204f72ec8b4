// exact_limited_move.hip -- exact_limited.hip on the fourteen features: tpl_placement_exact_limited_move.
#define TPL_PLACEMENT_MOVE_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#define TPL_EXACT_LIMITED_UNIT
#include "exact.hip"
