#!/usr/bin/env python3
"""DDPG on N vectorised reach_ball envs with a continuous action, everything on the GPU.

Mirror of the reference's ddpg_stable_baselines3.py (use_continuous_action=True, use_turning=False; --turning for the 4-D
variant) with stable-baselines3 -- which cannot be installed offline -- replaced by a small plain-torch DDPG: actor
Linear-ReLU-Linear-ReLU-Linear-Tanh (SB3's actor.mu with policy_kwargs=dict(net_arch=[64, 64])), critic Q(s, a), target nets
with Polyak averaging, Gaussian action noise, a replay buffer in device memory.

    python examples/ddpg_reach_ball.py --envs 4096 --iters 10 --train-steps 200 --test-steps 250 --fused-actor 32

--fused-actor T collects T x N transitions per launch: the engine evaluates the learner's own actor in-kernel
(Engine.rollout_actor with a soccer2d_amd.actor.DeterministicActor), with epsilon-random exploration for the first launches
(SB3's learning_starts) and Gaussian action noise; the actor's packed weights are refreshed with sync() after every optimiser
phase and Timeouts bootstrap from the recorded terminal observations.  0: one torch forward per step.
--fused-target computes the TD targets in one launch from the target actor and critic (soccer2d_amd.td.ActorCriticTarget,
INTEGRATION 3f) instead of a chain of torch ops, and reloads its buffers after every Polyak step.
--fused-learner runs the critic's and the actor's update in HIP (soccer2d_amd.learn.ActorCriticLearner): forward,
backward through the critic and Adam, three launches each, and the Polyak step as one lerp_ per network; the networks must be on
the learner's grid (1 to 4 hidden layers of multiples of 8 in [8, 256]), so SB3's [400, 300] stays with torch's optimisers.
"""
import argparse
import copy
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
    'use_continuous_action': True, 'action_space_size': 16, 'use_turning': False,
}


def mlp(n_in, n_out, hidden=64, tanh=False, net_arch=None, activation='relu'):
    """net_arch / activation: SB3's policy_kwargs=dict(net_arch=dict(pi=[16, 8], qf=[...]), activation_fn=nn.Tanh)"""
    act = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}[activation]
    layers = []
    for w in (net_arch or (hidden, hidden)):
        layers += [nn.Linear(n_in, w), act()]
        n_in = w
    layers.append(nn.Linear(n_in, n_out))
    return nn.Sequential(*(layers + ([nn.Tanh()] if tanh else [])))


class DeviceReplay:
    def __init__(self, capacity, n_obs, n_act, device):
        self.cap, self.pos, self.full = capacity, 0, False
        self.obs = torch.empty((capacity, n_obs), device=device)
        self.next_obs = torch.empty((capacity, n_obs), device=device)
        self.act = torch.empty((capacity, n_act), device=device)
        self.rew = torch.empty((capacity,), device=device)
        self.term = torch.empty((capacity,), device=device)

    def add(self, obs, act, rew, next_obs, term):
        n = obs.shape[0]
        idx = (torch.arange(n, device=obs.device) + self.pos) % self.cap
        self.obs[idx], self.act[idx], self.rew[idx], self.next_obs[idx], self.term[idx] = obs, act, rew, next_obs, term
        self.full |= self.pos + n >= self.cap
        self.pos = (self.pos + n) % self.cap

    def sample(self, batch):
        hi = self.cap if self.full else self.pos
        i = torch.randint(0, hi, (batch,), device=self.obs.device)
        return self.obs[i], self.act[i], self.rew[i], self.next_obs[i], self.term[i]


class DeviceDDPG:
    def __init__(self, env, lr=1e-3, gamma=0.99, tau=0.005, buffer=1 << 20, batch=4096, grad_steps=1, sigma=0.1,
                 learning_starts=2, seed=0, net_arch=None, activation='relu', n_step=1, per_alpha=0.0, per_beta=0.4,
                 fused_target=False, fused_learner=False):
        torch.manual_seed(seed)
        self.fused_target, self.fused_learner, self.lr = fused_target, fused_learner, lr
        self.buffer, self.n_step, self.seed = buffer, n_step, seed
        self.per_alpha, self.per_beta = per_alpha, per_beta             # alpha 0: the uniform DeviceReplay
        self.env, self.dev = env, env.device
        n_obs, self.n_act = env.observation_space.shape[0], env.action_space.shape[0]
        self.general = net_arch is not None or activation != 'relu'      # an actor only the general fused actor takes
        self.mu = mlp(n_obs, self.n_act, tanh=True, net_arch=net_arch, activation=activation).to(self.dev)
        self.q = mlp(n_obs + self.n_act, 1).to(self.dev)
        self.mu_target, self.q_target = copy.deepcopy(self.mu), copy.deepcopy(self.q)
        self.opt_mu = torch.optim.Adam(self.mu.parameters(), lr=lr)
        self.opt_q = torch.optim.Adam(self.q.parameters(), lr=lr)
        self.rb = DeviceReplay(buffer, n_obs, self.n_act, self.dev)
        self.gamma, self.tau, self.batch, self.grad_steps, self.sigma = gamma, tau, batch, grad_steps, sigma
        self.learning_starts, self.launches = learning_starts, 0
        self.obs = env.reset().clone()

    @torch.no_grad()
    def predict(self, obs, noise=False):
        a = self.mu(obs)
        if noise:
            a = (a + self.sigma * torch.randn_like(a)).clamp(-1, 1)
        return a

    def optimise(self, n_updates, fused=False):
        """fused: batches of the fused path's soccer2d_amd.replay.DeviceReplay (reward = the n-step return, discount = gamma^k
        or 0) instead of the per-step buffer's (obs, action, reward, next_obs, term).  With --per-alpha that buffer is a
        PrioritizedReplay: the critic's loss carries the importance weights and the batch's slots get (|TD error| + 1e-6) ** alpha
        as their new priority."""
        per = fused and self.per_alpha > 0
        if fused and self.fused_learner:
            return self.optimise_fused(n_updates, per)
        for _g in range(n_updates):
            if fused:
                b = self.frb.sample(self.batch, out=self.fbatch)
                o, a, r, no, disc = b['obs'], b['action'], b['reward'], b['next_obs'], b['discount']
            else:
                o, a, r, no, t = self.rb.sample(self.batch)
                disc = self.gamma * (1 - t)
            if fused and self.fused_target:                      # one launch: the target actor and the target critic on the batch
                tgt = self.td.target(b, out=self.ftgt)
            else:
                with torch.no_grad():
                    tgt = r + disc * self.q_target(torch.cat([no, self.mu_target(no)], 1)).squeeze(1)
            q_sa = self.q(torch.cat([o, a], 1)).squeeze(1)
            if per:
                td = q_sa - tgt
                loss_q = (self.frb.weights(b, self.per_beta) * td * td).mean()
                self.frb.update_priorities(b['index'], (td.detach().abs() + 1e-6) ** self.per_alpha)
            else:
                loss_q = nn.functional.mse_loss(q_sa, tgt)
            self.opt_q.zero_grad(set_to_none=True)
            loss_q.backward()
            self.opt_q.step()
            loss_mu = -self.q(torch.cat([o, self.mu(o)], 1)).mean()
            self.opt_mu.zero_grad(set_to_none=True)
            loss_mu.backward()
            self.opt_mu.step()
            with torch.no_grad():
                for net, tgt_net in ((self.mu, self.mu_target), (self.q, self.q_target)):
                    for p, pt in zip(net.parameters(), tgt_net.parameters()):
                        pt.mul_(1 - self.tau).add_(p, alpha=self.tau)
            if fused and self.fused_target:
                self.td.sync()                                   # the next target launch reads the Polyak-averaged weights

    def optimise_fused(self, n_updates, per):
        """--fused-learner: sample -> target -> the critic's step -> the actor's step -> the Polyak step, the two steps in HIP"""
        for _g in range(n_updates):
            b = self.frb.sample(self.batch, out=self.fbatch)
            if self.fused_target:
                tgt = self.td.target(b, out=self.ftgt)
            else:
                with torch.no_grad():
                    no = b['next_obs']
                    tgt = b['reward'] + b['discount'] * self.q_target(torch.cat([no, self.mu_target(no)], 1)).squeeze(1)
            if per:
                self.learner.step(b, tgt, weight=self.frb.weights(b, self.per_beta), td_abs_out=self.fabs)
                self.frb.update_priorities(b['index'], (self.fabs + 1e-6) ** self.per_alpha)
            else:
                self.learner.step(b, tgt)
            if self.fused_target:
                self.learner.update_targets(self.td, self.tau)   # flat buffer to flat buffer; the target modules follow
            else:
                with torch.no_grad():
                    for net, tgt_net in ((self.mu, self.mu_target), (self.q, self.q_target)):
                        for p, pt in zip(net.parameters(), tgt_net.parameters()):
                            pt.mul_(1 - self.tau).add_(p, alpha=self.tau)

    def make_fused_learner(self):
        """--fused-learner: the learner takes over mu's and q's parameters (they become views of its flat buffers), made once"""
        if self.fused_learner and not hasattr(self, 'learner'):
            from soccer2d_amd.learn import ActorCriticLearner
            try:
                self.learner = ActorCriticLearner.from_modules(self.mu, self.q, actor_lr=self.lr, critic_lr=self.lr,
                                                               max_batch=self.batch, device=self.dev)
            except ValueError as e:
                raise SystemExit(f'--fused-learner: {e}.  The learner\'s grid is 1 to 4 hidden layers of multiples of 8 in [8, 256] '
                                 'with ReLU, Tanh or Sigmoid, at most 248 observation words and 8 actions; run this network without '
                                 '--fused-learner') from None
            self.fabs = torch.empty((self.batch,), dtype=torch.float32, device=self.dev)

    def _store(self, obs_t, act, rec_obs, rew, done, res, term_obs):
        next_obs = torch.where(done.bool().unsqueeze(-1), term_obs, rec_obs)            # bootstrap through Timeouts
        term = ((res == 1) | (res == 2)).float()                                          # Goal / Out are true terminations
        d = obs_t.shape[-1]
        self.rb.add(obs_t.reshape(-1, d), act.reshape(-1, self.n_act), rew.reshape(-1), next_obs.reshape(-1, d), term.reshape(-1))

    def learn(self, vec_steps):
        """one torch forward per vector step (the torch-in-the-loop path)"""
        for _ in range(vec_steps):
            if self.launches < self.learning_starts:
                act = torch.rand((self.env.num_envs, self.n_act), device=self.dev) * 2 - 1
            else:
                act = self.predict(self.obs, noise=True)
            nobs, rew, done, info = self.env.step(act)
            self._store(self.obs, act, nobs, rew, done, info['result'], info['terminal_observation'])
            self.obs = nobs.clone()
            if self.rb.full or self.rb.pos >= self.batch:
                self.optimise(self.grad_steps)
        self.launches += 1

    def learn_fused(self, vec_steps, T):
        """The same DDPG, experience collected T steps per launch by the fused actor (the learner's own actor in-kernel):
        epsilon = 1 (uniform random actions) for the first learning_starts launches, then the noisy actor."""
        from soccer2d_amd.actor import DeterministicActor
        from soccer2d_amd.mlp_actor import MlpDeterministicActor
        from soccer2d_amd.wide_actor import WideDeterministicActor
        if not hasattr(self, 'actor'):
            kw = dict(device=self.dev, epsilon=1.0, noise_sigma=self.sigma)
            if not self.general:
                self.actor = DeterministicActor.from_module(self.mu, **kw)
            else:
                try:
                    self.actor = MlpDeterministicActor.from_module(self.mu, **kw)
                except ValueError:      # SB3's default [400, 300], five layers, Sigmoid, or too large for the LDS: streamed weights
                    self.actor = WideDeterministicActor.from_module(self.mu, **kw)
            print(f'fused actor: {type(self.actor).__name__}')
            self.rec = self.env.engine.alloc_rollout(T, terminal_obs=True)
        self.make_fused_target()
        self.make_fused_learner()
        eng, rec = self.env.engine, self.rec
        rb = self.fused_replay(T, eng.obs.shape[-1])
        for _ in range((vec_steps + T - 1) // T):
            self.actor.epsilon = 1.0 if self.launches < self.learning_starts else 0.0
            obs0 = eng.obs.clone()                               # the observation the first action is chosen from
            self.env.rollout(T, out=rec, policy=self.actor, terminal_obs=True)
            rb.push(rec, obs0)                                   # T x N n-step transitions, Timeouts bootstrap (one launch)
            self.after_fused_launch(T)
        self.obs = eng.obs.clone()

    def make_fused_target(self):
        """--fused-target: the target launch's state (soccer2d_amd.td.ActorCriticTarget) and the tensor it writes, made once"""
        if self.fused_target and not hasattr(self, 'td'):
            from soccer2d_amd.td import ActorCriticTarget
            self.td = ActorCriticTarget.from_modules(self.mu_target, self.q_target, device=self.dev)
            self.ftgt = torch.empty((self.batch,), dtype=torch.float32, device=self.dev)

    def fused_replay(self, T, n_obs):
        """the device replay buffer of the fused path (soccer2d_amd.replay.DeviceReplay, or PrioritizedReplay with --per-alpha),
        made at the first launch: it holds at least one record"""
        from soccer2d_amd.replay import DeviceReplay as UniformReplay, PrioritizedReplay
        FusedReplay = PrioritizedReplay if self.per_alpha > 0 else UniformReplay
        if not hasattr(self, 'frb'):
            self.frb = FusedReplay(max(self.buffer, T * self.env.num_envs), n_obs, self.n_act, torch.float32, self.dev,
                                   n_step=self.n_step, gamma=self.gamma, seed=self.seed)
            self.fbatch, self.stored = self.frb.alloc_batch(self.batch), 0
        return self.frb

    def after_fused_launch(self, T):
        self.launches += 1
        self.stored += T * self.env.num_envs
        if self.stored >= self.batch:
            self.optimise(self.grad_steps * T, fused=True)
            self.actor.sync()                                    # the next launch acts with the new weights


def test(env, model, vec_steps):
    """deterministic policy (no noise), count info['result'] of finished episodes"""
    obs = env.reset()
    counts = torch.zeros(4, dtype=torch.int64, device=env.device)
    for _ in range(vec_steps):
        act = model.predict(obs) if model is not None else None
        obs, rew, done, info = env.step(act)
        counts += torch.bincount(info['result'].long(), minlength=4)
    c = counts.cpu().tolist()
    n = max(1, c[1] + c[2] + c[3])
    return {'Goal': c[1] / n, 'Out': c[2] / n, 'Timeout': c[3] / n, 'episodes': n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--train-steps', type=int, default=200)
    ap.add_argument('--test-steps', type=int, default=250)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--turning', action='store_true', help='use_turning=True: the 4-D action')
    ap.add_argument('--fused-actor', type=int, default=0, metavar='T',
                    help='collect T steps per launch with the in-kernel actor (0: one torch forward per step)')
    ap.add_argument('--net-arch', default=None, metavar='W1,W2,...',
                    help="the actor's hidden widths, e.g. 16,8 or 400,300 (1 to 5 multiples of 4 up to 400; default: 64,64)")
    ap.add_argument('--activation', choices=('relu', 'tanh', 'sigmoid'), default='relu')
    ap.add_argument('--n-step', type=int, default=1, metavar='K', help='with --fused-actor: K-step returns in the replay buffer')
    ap.add_argument('--per-alpha', type=float, default=0.0, metavar='A',
                    help='with --fused-actor: prioritized replay, priority = (|TD error| + 1e-6) ** A (0: uniform sampling)')
    ap.add_argument('--fused-target', action='store_true',
                    help='with --fused-actor: the TD targets in one launch from the target actor and critic '
                         '(soccer2d_amd.td.ActorCriticTarget)')
    ap.add_argument('--per-beta', type=float, default=0.4, metavar='B', help='with --per-alpha: the importance-weight exponent')
    ap.add_argument('--fused-learner', action='store_true',
                    help="with --fused-actor: the critic's and the actor's update in HIP (soccer2d_amd.learn.ActorCriticLearner)")
    args = ap.parse_args()
    if args.fused_target and args.fused_actor <= 0:
        ap.error('--fused-target needs --fused-actor T')
    if args.fused_learner and args.fused_actor <= 0:
        ap.error('--fused-learner needs --fused-actor T')
    net_arch = [int(w) for w in args.net_arch.split(',')] if args.net_arch else None
    kw = dict(kewargs, use_turning=args.turning)
    env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, **kw)
    test_env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, seed=1234, **kw)
    model = DeviceDDPG(env, net_arch=net_arch, activation=args.activation, n_step=args.n_step, per_alpha=args.per_alpha,
                       per_beta=args.per_beta, fused_target=args.fused_target, fused_learner=args.fused_learner)
    r0 = test(test_env, model, args.test_steps)
    print('untrained actor:', r0)
    r = r0
    for i in range(args.iters):
        t0 = time.time()
        if args.fused_actor > 0:
            model.learn_fused(args.train_steps, args.fused_actor)
        else:
            model.learn(args.train_steps)
        torch.cuda.synchronize()
        dt = time.time() - t0
        r = test(test_env, model, args.test_steps)
        print(f'iter {i}: {args.train_steps * args.envs / dt / 1e6:.2f} M env-steps/s incl. learning  {r}')
    print(f"goal share: {r0['Goal']:.4f} before, {r['Goal']:.4f} after {args.iters} iterations")
    env.close(); test_env.close()


if __name__ == '__main__':
    main()
