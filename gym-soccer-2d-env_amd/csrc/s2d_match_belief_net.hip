// s2d_match_belief_net.hip -- the belief-network instantiations of the 11v11 cycle kernel ("Belief network", include/s2d_match.h).
//
// A translation unit of its own, for the reasons s2d_match_see_policy.hip gives: the BEL family is five more instantiations of
// the library's largest kernel, which compile beside s2d_match.hip instead of after it, and nothing instantiated here can reach
// the code of the SEE and SEEPOL kernels it was derived from.
//
// The cycle kernel, its device functions and the launch plumbing come from s2d_match_host.h and the headers under it (the belief
// update: s2d_belief_row.h, the update of s2d_belief.hip's scan kernel as a device function); what may exist only once in the library is in
// s2d_match.hip.  This unit defines one function, the launch s2d_match.hip's m_launch calls when the engine holds a belief network.
#include "s2d_match_host.h"

int s2d_match_internal_belief_net_launch(S2DMatchHandle h, int n_steps, const float* actions, const MRoll& ro, hipStream_t st,
                                         const MCtl& ctl, const MBelArg& ba) {
  return m_dispatch<true, true>(h, n_steps, actions, ro, st, ctl, ba);
}
