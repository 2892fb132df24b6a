// s2d_match_reward.hip -- the agent-reward instantiations of the 11v11 cycle kernel ("Agent reward", include/s2d_match.h).
//
// A translation unit of its own, for two reasons.  The RW family is 15 more instantiations of the library's largest kernel: built
// beside s2d_match.hip they compile in parallel with it.  And nothing instantiated here can reach the code of s2d_match.hip's
// kernels: helpers that two families share have been optimised differently before (see MParamsCtl in s2d_match_rules.h).
//
// The cycle kernel, its device functions and the launch plumbing come from s2d_match_host.h and the headers under it; what may
// exist only once in the library -- the non-template kernels and the C ABI -- is in s2d_match.hip.  This unit defines one
// function, the launch s2d_match.hip's m_launch calls when a reward record is asked for.
#include "s2d_match_host.h"

// na: the network launch (one or two Q-networks, or records only); pa: the policy launch; neither: the controller launch.
int s2d_match_internal_reward_launch(S2DMatchHandle h, int n_steps, const float* actions, const MRoll& ro, hipStream_t st, const MCtlRw& ctl,
                                     const MNetArg* na, const MPolArg* pa) {
  if (pa) return m_dispatch<true, true>(h, n_steps, actions, ro, st, ctl, *pa);
  if (na) return m_dispatch<true, true>(h, n_steps, actions, ro, st, ctl, *na);
  return m_dispatch<true>(h, n_steps, actions, ro, st, ctl);
}
