// The tracking instances (TRK: per-problem, per-knot goals from the goal window, tmpc_set_reference) of
// tmpc_fd.hip's line-search kernel, as a translation unit of their own: they are as many as the fixed-goal
// instances, and the two sets build side by side.
#define TMPC_TRK_PART
#include "tmpc_fd.hip"
