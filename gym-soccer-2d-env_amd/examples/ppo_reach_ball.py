#!/usr/bin/env python3
"""PPO on N vectorised reach_ball envs, everything on the GPU.

stable-baselines3 -- which cannot be installed offline -- is replaced by a small plain-torch PPO of the same shape: a policy
net Linear-F-Linear-F-Linear (F = ReLU, or Tanh with --tanh: SB3's MlpPolicy default) whose outputs are the logits of a
categorical policy (the default, 16 discrete actions) or the means of a diagonal Gaussian with a state-independent log_std
(--continuous: 1-D, --turning: 4-D), a separate value net, GAE and clipped-surrogate minibatch epochs.

    python examples/ppo_reach_ball.py --envs 4096 --iters 20 --fused-actor 32 --tanh

--fused-actor T collects T x N transitions per launch: the engine samples from the learner's own policy in-kernel and records
the log-probabilities (Engine.rollout_policy with a soccer2d_amd.actor.StochasticActor).  The VALUE net stays in torch on
purpose: one batched forward over the recorded [T, N, 10] observations, the last observation and the terminal observations of
Timeouts is one large GEMM, while an in-kernel value network would double the network's share of every cycle for nothing.
Then soccer2d_amd.gae.gae() (one launch, Timeouts bootstrapped as SB3 does) and the epochs; the packed weights and log_std are
refreshed with sync() after them.  0: one torch forward per step (Categorical / Normal in the loop).

--fused-learner runs the epochs in HIP as well (soccer2d_amd.learn.PPOLearner): every minibatch step -- the gather by the
permutation, both forward passes, log-probability, entropy, clipped surrogate, value loss, backward, clip and Adam -- is one call,
and pi, vf and log_std stay the modules the rest of the script uses (their parameters become views of the learner's buffer).

--episode-stats (with --fused-actor) hands every collected record to soccer2d_amd.episodes.EpisodeStats (one more call per
launch, no host loop) and prints SB3's ep_rew_mean / ep_len_mean of the training episodes after each iteration.  --fused-eval T
evaluates with the same machinery instead of one torch forward and one env.step per vector step: the greedy policy in-kernel
(the learner's StochasticActor with deterministic = True) on the test env, T steps per launch, episodes counted on the device.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sample_environments.environment_factory import EnvironmentFactory  # noqa: E402

kewargs = {
    'change_ball_position': True, 'change_ball_velocity': True,
    'ball_position_x': 0, 'ball_position_y': 0, 'ball_speed': 0, 'ball_direction': 0,
    'min_distance_to_ball': 5.0, 'max_steps': 200,
    'use_continuous_action': False, 'action_space_size': 16, 'use_turning': False,
}
TIMEOUT = 3                                                # S2D_RESULT_TIMEOUT


def mlp(n_in, n_out, act, hidden=64):
    return nn.Sequential(nn.Linear(n_in, hidden), act(), nn.Linear(hidden, hidden), act(), nn.Linear(hidden, n_out))


class DevicePPO:
    def __init__(self, env, tanh=False, lr=3e-4, gamma=0.99, lam=0.95, clip=0.2, epochs=4, minibatches=4, vf_coef=0.5,
                 ent_coef=0.0, seed=0, hidden=64, fused_learner=False, max_batch=0):
        torch.manual_seed(seed)
        self.env, self.dev = env, env.device
        n_obs = env.observation_space.shape[0]
        self.discrete = hasattr(env.action_space, 'n')
        self.n_out = int(env.action_space.n) if self.discrete else env.action_space.shape[0]
        act = nn.Tanh if tanh else nn.ReLU
        self.pi = mlp(n_obs, self.n_out, act, hidden).to(self.dev)
        self.vf = mlp(n_obs, 1, act, hidden).to(self.dev)
        self.log_std = nn.Parameter(torch.zeros(self.n_out, device=self.dev))
        params = list(self.pi.parameters()) + list(self.vf.parameters()) + ([] if self.discrete else [self.log_std])
        self.learner = None
        if fused_learner:                                    # torch.optim.Adam's defaults and no gradient clip, as the torch arm
            from soccer2d_amd.learn import PPOLearner
            self.learner = PPOLearner.from_modules(self.pi, self.vf, log_std=None if self.discrete else self.log_std, lr=lr, eps=1e-8,
                                                   max_grad_norm=0.0, clip_range=clip, vf_coef=vf_coef, ent_coef=ent_coef,
                                                   max_batch=(max_batch + minibatches - 1) // minibatches)
        else:
            self.opt = torch.optim.Adam(params, lr=lr)
        self.gamma, self.lam, self.clip, self.epochs, self.minibatches = gamma, lam, clip, epochs, minibatches
        self.vf_coef, self.ent_coef = vf_coef, ent_coef
        self.obs = env.reset().clone()
        self.last_loss = float('nan')
        self.episode_stats = None                            # --episode-stats: an EpisodeStats the collected records go through

    def dist(self, obs):
        y = self.pi(obs)
        if self.discrete:
            return torch.distributions.Categorical(logits=y)
        return torch.distributions.Independent(torch.distributions.Normal(y, self.log_std.exp().expand_as(y)), 1)

    @torch.no_grad()
    def predict(self, obs):
        """the greedy action (evaluation)"""
        y = self.pi(obs)
        return y.argmax(-1) if self.discrete else y.clamp(-1, 1)

    def update(self, obs, act, logp_old, adv, ret):
        """clipped-surrogate epochs over the flattened batch"""
        B = obs.shape[0]
        mb = (B + self.minibatches - 1) // self.minibatches
        if self.learner is not None:                         # the same epochs, a minibatch step per call, the gather in the kernel
            ro = {'obs': obs, 'action': act.int() if self.discrete else act, 'logp': logp_old, 'advantage': adv, 'return': ret}
            for _e in range(self.epochs):
                perm = torch.randperm(B, device=self.dev).int()
                for s in range(0, B, mb):
                    self.learner.step(ro, perm[s:s + mb])
            self.last_loss = self.learner.loss
            return
        for _e in range(self.epochs):
            perm = torch.randperm(B, device=self.dev)
            for s in range(0, B, mb):
                i = perm[s:s + mb]
                d = self.dist(obs[i])
                logp = d.log_prob(act[i])
                a = adv[i]
                a = (a - a.mean()) / (a.std() + 1e-8)
                ratio = (logp - logp_old[i]).exp()
                pg = -torch.min(ratio * a, ratio.clamp(1 - self.clip, 1 + self.clip) * a).mean()
                v_loss = nn.functional.mse_loss(self.vf(obs[i]).squeeze(-1), ret[i])
                loss = pg + self.vf_coef * v_loss - self.ent_coef * d.entropy().mean()
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self.opt.step()
        self.last_loss = float(loss.detach())

    def _finish(self, obs_t, act, logp, rew, done, res, term_obs, last_obs):
        """values in ONE batched forward (record, last observation, terminal observations), then gae() and the epochs"""
        from soccer2d_amd.gae import gae
        T, N, D = obs_t.shape
        with torch.no_grad():
            v = self.vf(torch.cat([obs_t.reshape(-1, D), last_obs, term_obs.reshape(-1, D).nan_to_num()])).squeeze(-1)
        value, last_value, tval = v[:T * N].reshape(T, N), v[T * N:T * N + N].contiguous(), v[T * N + N:].reshape(T, N)
        adv, ret = gae(rew, done, value.contiguous(), last_value, self.gamma, self.lam, result=res, terminal_value=tval.contiguous())
        a = act.reshape(T * N) if self.discrete else act.reshape(T * N, self.n_out)
        self.update(obs_t.reshape(-1, D), a, logp.reshape(-1), adv.reshape(-1), ret.reshape(-1))

    def learn(self, vec_steps, T):
        """one torch forward per vector step (the torch-in-the-loop path), T steps per update"""
        N, D = self.env.num_envs, self.obs.shape[-1]
        f = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=self.dev)
        for _ in range((vec_steps + T - 1) // T):
            obs_t, rew, logp, term = f(T, N, D), f(T, N), f(T, N), f(T, N, D)
            act = f(T, N, dt=torch.int64) if self.discrete else f(T, N, self.n_out)
            done, res = f(T, N, dt=torch.uint8), f(T, N, dt=torch.uint8)
            for t in range(T):
                with torch.no_grad():
                    d = self.dist(self.obs)
                    a = d.sample()
                    logp[t] = d.log_prob(a)
                nobs, r, dn, info = self.env.step(a if self.discrete else a.clamp(-1, 1))
                obs_t[t], act[t], rew[t], done[t], res[t], term[t] = self.obs, a, r, dn, info['result'], info['terminal_observation']
                self.obs = nobs.clone()
            self._finish(obs_t, act, logp, rew, done, res, term, self.obs)

    def fused_actor(self):
        """the in-kernel policy (the learner's own policy net), made once"""
        from soccer2d_amd.actor import StochasticActor
        if not hasattr(self, 'actor'):
            self.actor = StochasticActor.from_module(self.pi, log_std=None if self.discrete else self.log_std, device=self.dev)
        return self.actor

    def learn_fused(self, vec_steps, T):
        """The same PPO, experience collected T steps per launch by the fused stochastic policy (the learner's own policy net
        in-kernel, with the log-probabilities recorded)."""
        if not hasattr(self, 'rec'):
            self.fused_actor()
            self.rec = self.env.engine.alloc_rollout(T, terminal_obs=True, logp=True)
            self.rec['terminal_obs'].zero_()
        eng, rec = self.env.engine, self.rec
        for _ in range((vec_steps + T - 1) // T):
            obs0 = eng.obs.clone()                               # the observation the first action is chosen from
            self.env.rollout(T, out=rec, policy=self.actor, terminal_obs=True)
            if self.episode_stats is not None:
                self.episode_stats.update_record(rec)            # returns, lengths and results of the episodes that ended
            obs_t = torch.cat([obs0[None], rec['obs'][:-1]])       # action t was chosen from the observation of step t - 1
            self._finish(obs_t, rec['action'].long() if self.discrete else rec['action'], rec['logp'], rec['reward'], rec['done'],
                         rec['result'], rec['terminal_obs'], eng.obs)
            self.actor.sync()                                    # the next launch samples from the new policy
        self.obs = eng.obs.clone()


def test(env, model, vec_steps):
    """greedy policy, count info['result'] of finished episodes"""
    obs = env.reset()
    counts = torch.zeros(4, dtype=torch.int64, device=env.device)
    for _ in range(vec_steps):
        obs, rew, done, info = env.step(model.predict(obs))
        counts += torch.bincount(info['result'].long(), minlength=4)
    c = counts.cpu().tolist()
    n = max(1, c[1] + c[2] + c[3])
    return {'Goal': c[1] / n, 'Out': c[2] / n, 'Timeout': c[3] / n, 'episodes': n}


def test_fused(env, model, vec_steps, T):
    """test() without the per-step loop: the greedy policy in-kernel on the test env, T steps per launch, and the finished
    episodes counted by an EpisodeStats that keeps every one of them; test()'s keys plus ep_rew_mean / ep_len_mean"""
    from soccer2d_amd.episodes import EpisodeStats
    env.reset()
    eng, actor = env.engine, model.fused_actor()
    actor.sync()                                             # the weights as they are now
    stats = EpisodeStats(env.num_envs, capacity=vec_steps * env.num_envs, device=env.device)
    rec = eng.alloc_rollout(T, with_obs=False)
    was, actor.deterministic = actor.deterministic, True
    try:
        for t in range(0, vec_steps, T):
            n = min(T, vec_steps - t)
            eng.rollout_policy(n, actor, out=rec, with_obs=False, logp=False)
            stats.update(rec['reward'][:n], rec['done'][:n], rec['result'][:n])
    finally:
        actor.deterministic = was
    s = stats.summary()
    return {'Goal': s['Goal'], 'Out': s['Out'], 'Timeout': s['Timeout'], 'episodes': max(1, s['episodes']),
            'ep_rew_mean': s['ep_rew_mean'], 'ep_len_mean': s['ep_len_mean']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--train-steps', type=int, default=128)
    ap.add_argument('--test-steps', type=int, default=250)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--tanh', action='store_true', help='Tanh hidden activations (SB3\'s MlpPolicy default) instead of ReLU')
    ap.add_argument('--continuous', action='store_true', help='use_continuous_action=True: a 1-D Gaussian policy')
    ap.add_argument('--turning', action='store_true', help='use_turning=True: the 4-D Gaussian policy')
    ap.add_argument('--fused-actor', type=int, default=0, metavar='T',
                    help='collect T steps per launch with the in-kernel policy (0: one torch forward per step, 32 per update)')
    ap.add_argument('--fused-learner', action='store_true',
                    help='the minibatch epochs in HIP (soccer2d_amd.learn.PPOLearner) instead of torch autograd and Adam')
    ap.add_argument('--hidden', type=int, default=64, help='width of the two hidden layers of both networks (64; another width shows what --fused-learner and --fused-actor '
                         'accept: the learner takes multiples of 8 in [8, 256] and names that grid when it refuses)')
    ap.add_argument('--episode-stats', action='store_true',
                    help='with --fused-actor: episode returns / lengths / results of the collected records on the device '
                         '(soccer2d_amd.episodes.EpisodeStats), one more line per iteration')
    ap.add_argument('--fused-eval', type=int, default=0, metavar='T',
                    help='evaluate with the in-kernel greedy policy, T steps per launch, episodes counted on the device '
                         '(0: one torch forward and one env.step per vector step)')
    args = ap.parse_args()
    if args.episode_stats and args.fused_actor <= 0:
        ap.error('--episode-stats needs --fused-actor T')
    kw = dict(kewargs, use_continuous_action=args.continuous or args.turning, use_turning=args.turning)
    env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, **kw)
    test_env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, seed=1234, **kw)
    model = DevicePPO(env, tanh=args.tanh, hidden=args.hidden, fused_learner=args.fused_learner,
                      max_batch=args.envs * (args.fused_actor if args.fused_actor > 0 else 32))
    if args.episode_stats:
        from soccer2d_amd.episodes import EpisodeStats
        model.episode_stats = EpisodeStats(args.envs, device=env.device)      # SB3's window of 100 episodes
    evaluate = (lambda: test_fused(test_env, model, args.test_steps, args.fused_eval)) if args.fused_eval > 0 else \
        (lambda: test(test_env, model, args.test_steps))
    r0 = evaluate()
    print('untrained policy:', r0)
    r = r0
    for i in range(args.iters):
        t0 = time.time()
        if args.fused_actor > 0:
            model.learn_fused(args.train_steps, args.fused_actor)
        else:
            model.learn(args.train_steps, 32)
        torch.cuda.synchronize()
        dt = time.time() - t0
        r = evaluate()
        print(f'iter {i}: loss {model.last_loss:.5f}  {args.train_steps * args.envs / dt / 1e6:.2f} M env-steps/s incl. learning  {r}')
        if model.episode_stats is not None:
            s = model.episode_stats.summary()
            print(f"iter {i}: ep_rew_mean {s['ep_rew_mean']:.4f}  ep_len_mean {s['ep_len_mean']:.2f}  Goal {s['window_goal']:.4f} over the "
                  f"last {s['window']} of {s['episodes']} training episodes")
    print(f"goal share: {r0['Goal']:.4f} before, {r['Goal']:.4f} after {args.iters} iterations")
    env.close(); test_env.close()


if __name__ == '__main__':
    main()
