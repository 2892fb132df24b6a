// s2d_match_see_policy.hip -- the see-policy instantiations of the 11v11 cycle kernel ("See policy slots", include/s2d_match.h).
//
// A translation unit of its own, for the reasons s2d_match_reward.hip gives: the SEEPOL family is five more instantiations of
// the library's largest kernel, which compile beside s2d_match.hip instead of after it, and nothing instantiated here can reach
// the code of the SEE kernels it was derived from.
//
// The cycle kernel, its device functions and the launch plumbing come from s2d_match_host.h and the headers under it; what may
// exist only once in the library -- the non-template kernels and the C ABI -- is in s2d_match.hip.  This unit defines one
// function, the launch s2d_match.hip's m_launch calls when the engine's see network holds a policy.
#include "s2d_match_host.h"

int s2d_match_internal_see_policy_launch(S2DMatchHandle h, int n_steps, const float* actions, const MRoll& ro, hipStream_t st,
                                         const MCtl& ctl, const MSeePolArg& pa) {
  return m_dispatch<true, true>(h, n_steps, actions, ro, st, ctl, pa);
}
