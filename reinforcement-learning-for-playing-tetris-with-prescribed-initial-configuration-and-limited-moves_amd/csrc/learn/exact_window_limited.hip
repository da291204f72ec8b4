// exact_window_limited.hip -- exact_window.hip once more, around the limited-discrepancy search: tpl_placement_window_prove_limited
// (include/tpl_learn.h states the rule; exact.hip says why this is a unit of its own).
#define TPL_EXACT_LIMITED_UNIT
#include "exact_window.hip"
