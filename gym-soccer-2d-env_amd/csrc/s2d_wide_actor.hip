// s2d_wide_actor.hip -- the fused actors on the streamed-weight MLP: the epsilon-greedy Q-network (s2d_rollout_qnet_wide) and the
// deterministic tanh policy with Gaussian action noise (s2d_rollout_actor_wide) with one to five hidden layers, widths that are
// multiples of 4 up to 400 and relu, tanh_spec or sigmoid_spec between them; include/s2d.h S2DWideNet, DESIGN.md sections 4, 5, 7.
//
// The rollout kernel is s2d_reach_actor_rollout_kernel (s2d_actor_rollout.h) over a second network back end (WideDims,
// s2d_wide_net.h): the heads, the draws, the simulation, the records and the statistics are the template's.  The weights do not
// live in LDS: the pack kernel (s2d_wide_pack.hip) writes them in fragment order into the caller's workspace, on the same stream
// ahead of the rollout, and the rollout's waves stream them from there (L2) into registers layer by layer.  The shape's checks,
// the workspace's, the plan and the diagnostic's host half are shared with the other users of the network (s2d_wide_host.h,
// s2d_wide_net.h, s2d_actor_rollout.h).  The activation and the env tiles
// per pass are fields of the kernel argument (wave-uniform), so the instantiations are those of the resident actors: 3 for the
// Q-actor, 12 for the tanh actor, and the diagnostic kernel.  On a shape the resident path takes the result is its, bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "s2d_actor_rollout.h"
#include "s2d_wide_net.h"

// host side (same library, hidden symbols; the rollouts' C entry points are in s2d_engine.hip, the tables and the launch in
// s2d_actor_rollout.h, s2d_wide_workspace_bytes and s2d_debug_wide_forward at the end of this file)
static const char kBytesFn[] = "s2d_wide_workspace_bytes";

// the plan of `net`'s shape: wide_net_plan with the observation's width and the rollout template's tail
static int wide_plan(const char* who, const S2DWideNet* net, ActorPlan<WideDims>& pl) {
  return wide_net_plan(who, net, S2D_OBS_DIM, kWideTail, pl.d, pl.wave_words, pl.waves, pl.lds);
}
int s2d_internal_wide_plan(const char* who, const S2DWideNet* net, ActorPlanBuf* buf) { return wide_plan(who, net, plan_in<WideDims>(buf)); }

// the workspace check, then the pack kernel and the rollout
int s2d_internal_rollout_wide(const ActorRollout& a, const char* who, const S2DWideNet* net, const ActorPlanBuf& buf) {
  ActorPlan<WideDims> pl = plan_of<WideDims>(buf);
  const WidePackArgs pack = wide_pack_args(pl.d, S2D_OBS_DIM);
  if (wide_net_workspace(who, net, pack, kBytesFn) != S2D_OK) return S2D_EINVAL;
  pl.d.wf = static_cast<const float*>(net->workspace);
  const float* const noise = net->noise_kind ? net->noise : nullptr;
  if (!launch_actor_rollout(a, pl, net->params, net->epsilon, noise,
                            [&] { s2d_internal_wide_pack(pack, net->params, net->workspace, static_cast<hipStream_t>(a.stream)); }))
    return -2;
  if (a.mode == S2D_MODE_DISCRETE)
    std::snprintf(a.name, a.name_bytes, "s2d_wide_qnet_rollout_kernel<noise=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>", a.nk,
                  kActName[net->activation], widths_text(net).c_str(), net->n_out, pl.waves, pl.d.tiles);
  else
    std::snprintf(a.name, a.name_bytes, "s2d_wide_actor_rollout_kernel<mode=%s,noise=%d,gauss=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>",
                  a.mode == S2D_MODE_TURN4 ? "turn4" : "cont1", a.nk, noise ? 1 : 0, kActName[net->activation], widths_text(net).c_str(),
                  net->n_out, pl.waves, pl.d.tiles);
  return 0;
}

S2D_API size_t s2d_wide_workspace_bytes(const S2DWideNet* shape) { return wide_net_workspace_bytes(shape, S2D_OBS_DIM); }

S2D_API int s2d_debug_wide_forward(const S2DWideNet* shape, const void* obs_dev, int64_t n, void* y_dev, void* greedy_dev, char* name,
                                   void* stream) {
  return debug_forward_streamed("s2d_debug_wide_forward", "s2d_debug_wide_forward_kernel", S2D_OBS_DIM, kBytesFn, wide_plan,
                                s2d_wide_debug_forward_kernel<S2D_OBS_DIM>, shape, obs_dev, n, y_dev, greedy_dev, name, stream);
}
