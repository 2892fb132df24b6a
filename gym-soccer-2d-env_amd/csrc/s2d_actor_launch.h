// s2d_actor_launch.h -- what the C entry points of the reach-ball engine's fused actors (s2d_engine.hip) and the three network
// back ends that launch for them (s2d_actor.hip, s2d_mlp_actor.hip, s2d_wide_actor.hip) say to each other: the launch arguments
// every back end takes alike, a back end's plan, and the back ends' functions (same library, hidden symbols).  Host code only.
#pragma once
#include <cstddef>
#include <cstdint>

#include "s2d_kernels.h"

// one fused-actor launch, as its entry point has checked it: the engine's side of the kernel arguments and where the kernel's
// name goes
struct ActorRollout {
  int mode, nk;                 // S2D_MODE_*, S2D_NK_* of the engine
  const S2DHot* hot;
  const S2DRare* rare_dev;
  float* S;
  int64_t stride, n;
  int n_steps;
  const RolloutOut* ro;
  float* term_rec;
  const StepOut* o;
  void* stream;
  char* name;
  size_t name_bytes;
};

// A back end's plan for one network, made once per launch by the entry point's call and handed to the launch.  The entry points
// only carry it: it is the back end's ActorPlan<Dims> (s2d_actor_rollout.h; the network headers define kernels and belong to one
// unit each).
struct ActorPlanBuf {
  alignas(8) unsigned char bytes[96];
};

// errors share the thread-local text of s2d_last_error() (defined in s2d_engine.hip)
extern "C" void s2d_internal_set_error(const char* msg);

// The launches: the Q head on a discrete engine, the tanh head on the others (`noise` non-NULL: with Gaussian action noise).
// 0, or -2 if hipGetDevice or hipFuncSetAttribute failed; nothing is enqueued unless 0 is returned.
// s2d_actor.hip: the plan of a 10-h1-h2-na network (false: it does not fit the LDS of a workgroup) and the launch with it
bool s2d_internal_net_plan(int h1, int h2, int na, ActorPlanBuf* pl);
int s2d_internal_rollout_net(const ActorRollout& a, const ActorPlanBuf& pl, const float* params, const float* eps, const float* noise);
// s2d_mlp_actor.hip / s2d_wide_actor.hip: the plan of `net`'s shape (everything but the engine's side of n_out and the pointers):
// S2D_OK, or S2D_EINVAL with the error text set (`who` = the entry point's name); and the launch with that plan.  The wide launch
// checks the workspace first (S2D_EINVAL with the text set).
int s2d_internal_mlp_plan(const char* who, const S2DMlpNet* net, ActorPlanBuf* pl);
int s2d_internal_rollout_mlp(const ActorRollout& a, const char* who, const S2DMlpNet* net, const ActorPlanBuf& pl);
int s2d_internal_wide_plan(const char* who, const S2DWideNet* net, ActorPlanBuf* pl);
int s2d_internal_rollout_wide(const ActorRollout& a, const char* who, const S2DWideNet* net, const ActorPlanBuf& pl);
// s2d_wide_actor.hip: the squashed-Gaussian (SAC) rollout on a network planned by s2d_internal_wide_plan (n_out = 2A); checks the
// workspace first, as the wide launch; 0, S2D_EINVAL with the text set, or -2
int s2d_internal_rollout_sac(const ActorRollout& a, const char* who, const S2DWideNet* net, const ActorPlanBuf& pl, const uint32_t* det,
                             float* logp);
// s2d_policy.hip: the stochastic policy rollout of any action mode on a network planned by s2d_internal_net_plan (act_fn = 0 relu | 1 tanh); 0 or -2
int s2d_internal_rollout_policy(const ActorRollout& a, const ActorPlanBuf& pl, int act_fn, const float* params, const float* log_std,
                                const uint32_t* det, float* logp);
