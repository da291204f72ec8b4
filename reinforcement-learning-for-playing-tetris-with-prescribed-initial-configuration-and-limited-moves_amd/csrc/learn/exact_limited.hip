// exact_limited.hip -- exact.hip once more, around the limited-discrepancy search: tpl_placement_exact_limited (include/tpl_learn.h
// states the rule; exact.hip says why this is a unit of its own).
#define TPL_EXACT_LIMITED_UNIT
#include "exact.hip"
