#!/usr/bin/env python3
"""Soft Actor-Critic on N vectorised reach_ball envs with a continuous action, everything on the GPU.

The off-policy companion of ddpg_reach_ball.py for use_continuous_action=True (--turning: the 4-D action), with
stable-baselines3 -- which cannot be installed offline -- replaced by a small plain-torch SAC: a squashed-Gaussian actor
Linear-(ReLU-Linear) x L with 2A outputs (SB3's actor.latent_pi, actor.mu and actor.log_std stacked; the log-std clamped to
[-20, 2]), twin critics Q(s, a) with Polyak-averaged targets, and the automatic entropy coefficient with target entropy -A.  The
replay buffer is soccer2d_amd.replay.DeviceReplay (n-step transitions on the device, Timeouts bootstrap).

    python examples/sac_reach_ball.py --envs 4096 --iters 10 --train-steps 256 --fused-actor 32 --fused-target

--fused-actor T collects T x N transitions per launch: the engine samples from the learner's own actor in-kernel
(Engine.rollout_sac with a soccer2d_amd.wide_actor.SquashedGaussianActor); its packed weights are refreshed with
sync() after every optimiser phase.  The first launches are the plain random rollout (SB3's learning_starts); it records no
terminal observations, so those launches store a Timeout as a termination.  0: one torch forward and one env.step per step.
--fused-target computes reward + discount * (min Q'(s', a') - alpha logp(a')) in one launch (soccer2d_amd.td.SacTarget): the
online actor's head draws a' with the kernel's own noise, alpha is read from a device word.
--fused-learner replaces the three torch optimiser steps and the Polyak loop by soccer2d_amd.learn.SACLearner: the critics' steps,
the actor's reparameterised step through min(Q1, Q2) and the temperature's step in HIP, with the learner's own noise; with
--fused-target the targets follow by SACLearner.update_targets and no sync() is needed inside the loop.  Without it the update is
plain torch.
"""
import argparse
import copy
import math
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sample_environments.environment_factory import EnvironmentFactory  # noqa: E402
from soccer2d_amd.replay import DeviceReplay  # noqa: E402

kewargs = {
    'change_ball_position': True, 'change_ball_velocity': True,
    'ball_position_x': 0, 'ball_position_y': 0, 'ball_speed': 0, 'ball_direction': 0,
    'min_distance_to_ball': 5.0, 'max_steps': 200,
    'use_continuous_action': True, 'action_space_size': 16, 'use_turning': False,
}
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0


def mlp(n_in, n_out, net_arch=(64, 64)):
    layers = []
    for w in net_arch:
        layers += [nn.Linear(n_in, w), nn.ReLU()]
        n_in = w
    return nn.Sequential(*layers, nn.Linear(n_in, n_out))


class DeviceSAC:
    def __init__(self, env, lr=3e-4, gamma=0.99, tau=0.005, buffer=1 << 20, batch=4096, learning_starts=1, seed=0, net_arch=(64, 64),
                 n_step=1, fused_target=False, fused_learner=False):
        torch.manual_seed(seed)
        self.env, self.dev = env, env.device
        n_obs, self.n_act = env.observation_space.shape[0], env.action_space.shape[0]
        self.actor = mlp(n_obs, 2 * self.n_act, net_arch).to(self.dev)       # rows 0 .. A-1 the means, A .. 2A-1 the raw log-std
        self.q1, self.q2 = mlp(n_obs + self.n_act, 1).to(self.dev), mlp(n_obs + self.n_act, 1).to(self.dev)
        self.q1_target, self.q2_target = copy.deepcopy(self.q1), copy.deepcopy(self.q2)
        self.log_alpha = torch.zeros(1, device=self.dev, requires_grad=True)
        self.alpha = torch.ones(1, device=self.dev)                         # the device word the fused target reads
        self.target_entropy = -float(self.n_act)
        self.opt_pi = torch.optim.Adam(self.actor.parameters(), lr=lr)
        self.opt_q = torch.optim.Adam(list(self.q1.parameters()) + list(self.q2.parameters()), lr=lr)
        self.opt_alpha = torch.optim.Adam([self.log_alpha], lr=lr)
        self.lrn = None
        if fused_learner:                                   # the modules' parameters become views of the learner's buffers
            from soccer2d_amd.learn import SACLearner
            self.lrn = SACLearner.from_modules(self.actor, self.q1, self.q2, ent_coef='auto', target_entropy=self.target_entropy,
                                               actor_lr=lr, critic_lr=lr, alpha_lr=lr, max_batch=batch, seed=seed, device=self.dev)
            self.alpha, self.log_alpha = self.lrn.alpha, self.lrn.log_alpha
        self.gamma, self.tau, self.batch, self.learning_starts, self.launches = gamma, tau, batch, learning_starts, 0
        self.buffer, self.n_step, self.seed, self.fused_target = buffer, n_step, seed, fused_target
        self.stored, self.losses = 0, None
        self.obs = env.reset().clone()

    def sample_action(self, obs):
        """(a = tanh(u), logp) with u ~ N(mean, exp(log_std)^2), reparameterised; SB3's log(1 - tanh^2 + 1e-6) correction"""
        mean, log_std = self.actor(obs).chunk(2, dim=1)
        log_std = log_std.clamp(LOG_STD_MIN, LOG_STD_MAX)
        z = torch.randn_like(mean)
        a = torch.tanh(mean + log_std.exp() * z)
        logp = (-0.5 * z * z - log_std - 0.5 * math.log(2 * math.pi) - torch.log(1 - a * a + 1e-6)).sum(dim=1)
        return a, logp

    @torch.no_grad()
    def predict(self, obs):
        return torch.tanh(self.actor(obs)[:, :self.n_act])

    def replay(self, T):
        """the device replay buffer, made at the first push: it holds at least one record"""
        if not hasattr(self, 'rb'):
            n_obs = self.obs.shape[-1]
            self.rb = DeviceReplay(max(self.buffer, T * self.env.num_envs), n_obs, self.n_act, torch.float32, self.dev,
                                   n_step=self.n_step, gamma=self.gamma, seed=self.seed)
            self.fbatch = self.rb.alloc_batch(self.batch)
            if self.fused_target:
                from soccer2d_amd.td import SacTarget
                self.td = SacTarget(self.actor, self.q1_target, self.q2_target, seed=self.seed, device=self.dev)
                self.ftgt = torch.empty((self.batch,), dtype=torch.float32, device=self.dev)
        return self.rb

    def optimise(self, n_updates):
        for _g in range(n_updates):
            b = self.rb.sample(self.batch, out=self.fbatch)
            o, a, r, no, disc = b['obs'], b['action'], b['reward'], b['next_obs'], b['discount']
            if self.fused_target:                                # one launch: the online actor's head and both target critics
                tgt = self.td.target(b, self.alpha, out=self.ftgt)
            else:
                with torch.no_grad():
                    na, nlogp = self.sample_action(no)
                    x = torch.cat([no, na], 1)
                    qn = torch.min(self.q1_target(x), self.q2_target(x)).squeeze(1)
                    tgt = r + disc * (qn - self.alpha * nlogp)
            if self.lrn is not None:                             # critics, then actor and temperature, in HIP
                self.lrn.step(b, tgt)
                if self.fused_target:
                    self.lrn.update_targets(self.td, self.tau)   # the Polyak step and the target's online actor: no sync()
                else:
                    with torch.no_grad():
                        for net, tgt_net in ((self.q1, self.q1_target), (self.q2, self.q2_target)):
                            for p, pt in zip(net.parameters(), tgt_net.parameters()):
                                pt.mul_(1 - self.tau).add_(p, alpha=self.tau)
                c1, c2 = self.lrn.critics
                self.losses = (c1.stats[0] + c2.stats[0], self.lrn.actor.stats[0], self.lrn.alpha_stats[1])
                continue
            x = torch.cat([o, a], 1)
            loss_q = 0.5 * (nn.functional.mse_loss(self.q1(x).squeeze(1), tgt) + nn.functional.mse_loss(self.q2(x).squeeze(1), tgt))
            self.opt_q.zero_grad(set_to_none=True)
            loss_q.backward()
            self.opt_q.step()
            a_pi, logp = self.sample_action(o)
            x = torch.cat([o, a_pi], 1)
            loss_pi = (self.alpha * logp - torch.min(self.q1(x), self.q2(x)).squeeze(1)).mean()
            self.opt_pi.zero_grad(set_to_none=True)
            loss_pi.backward()
            self.opt_pi.step()
            loss_alpha = -(self.log_alpha * (logp.detach() + self.target_entropy).mean())
            self.opt_alpha.zero_grad(set_to_none=True)
            loss_alpha.backward()
            self.opt_alpha.step()
            with torch.no_grad():
                self.alpha.copy_(self.log_alpha.exp())
                for net, tgt_net in ((self.q1, self.q1_target), (self.q2, self.q2_target)):
                    for p, pt in zip(net.parameters(), tgt_net.parameters()):
                        pt.mul_(1 - self.tau).add_(p, alpha=self.tau)
            if self.fused_target:
                self.td.sync()                                   # the next target launch reads the new actor and the Polyak step
            self.losses = (loss_q.detach(), loss_pi.detach(), loss_alpha.detach())

    def learn(self, vec_steps):
        """one torch forward and one env.step per vector step (the torch-in-the-loop path)"""
        rb = self.replay(1)
        for _ in range(vec_steps):
            if self.launches < self.learning_starts:
                act = torch.rand((self.env.num_envs, self.n_act), device=self.dev) * 2 - 1
            else:
                with torch.no_grad():
                    act = self.sample_action(self.obs)[0]
            nobs, rew, done, info = self.env.step(act)
            rec = {'obs': nobs.unsqueeze(0), 'terminal_obs': info['terminal_observation'].unsqueeze(0), 'action': act.unsqueeze(0),
                   'reward': rew.unsqueeze(0), 'done': done.unsqueeze(0), 'result': info['result'].unsqueeze(0)}
            rb.push({k: v.contiguous() for k, v in rec.items()}, self.obs)
            self.obs = nobs.clone()
            self.stored += self.env.num_envs
            if self.stored >= self.batch:
                self.optimise(1)
        self.launches += 1

    def learn_fused(self, vec_steps, T):
        """The same SAC, experience collected T steps per launch by the fused actor (the learner's own policy in-kernel); the
        first learning_starts launches are the plain random rollout."""
        from soccer2d_amd.wide_actor import SquashedGaussianActor
        eng = self.env.engine
        if not hasattr(self, 'fused'):
            self.fused = SquashedGaussianActor.from_module(self.actor, device=self.dev)
            self.rec = eng.alloc_rollout(T, terminal_obs=True, logp=True)
        rb, rec = self.replay(T), self.rec
        for _ in range((vec_steps + T - 1) // T):
            obs0 = eng.obs.clone()                               # the observation the first action is chosen from
            if self.launches < self.learning_starts:
                self.env.rollout(T, out=rec)                     # uniform random actions; no terminal observations are recorded
                rb.push(dict(rec, terminal_obs=rec['obs'], result=None), obs0)
            else:
                self.env.rollout(T, out=rec, policy=self.fused, terminal_obs=True)
                rb.push(rec, obs0)                               # T x N n-step transitions, Timeouts bootstrap (one launch)
            self.launches += 1
            self.stored += T * self.env.num_envs
            if self.stored >= self.batch:
                self.optimise(T)
                self.fused.sync()                                # the next launch acts with the new weights
        self.obs = eng.obs.clone()


def test(env, model, vec_steps):
    """deterministic policy (tanh of the mean), count info['result'] of finished episodes"""
    obs = env.reset()
    counts = torch.zeros(4, dtype=torch.int64, device=env.device)
    for _ in range(vec_steps):
        obs, rew, done, info = env.step(model.predict(obs))
        counts += torch.bincount(info['result'].long(), minlength=4)
    c = counts.cpu().tolist()
    n = max(1, c[1] + c[2] + c[3])
    return {'Goal': c[1] / n, 'Out': c[2] / n, 'Timeout': c[3] / n, 'episodes': n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--train-steps', type=int, default=256)
    ap.add_argument('--test-steps', type=int, default=250)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--turning', action='store_true', help='use_turning=True: the 4-D action')
    ap.add_argument('--fused-actor', type=int, default=0, metavar='T',
                    help='collect T steps per launch with the in-kernel squashed-Gaussian actor (0: one torch forward per step)')
    ap.add_argument('--fused-target', action='store_true',
                    help='the entropy-regularised TD targets in one launch (soccer2d_amd.td.SacTarget)')
    ap.add_argument('--fused-learner', action='store_true',
                    help='the critics\', the actor\'s and the temperature\'s steps in HIP (soccer2d_amd.learn.SACLearner: 1 to 4 hidden '
                         'widths, multiples of 8 in [8, 256])')
    ap.add_argument('--net-arch', default='64,64', metavar='W1,W2,...',
                    help="the actor's hidden widths, e.g. 256,256 (1 to 5 multiples of 4 in [8, 400])")
    ap.add_argument('--n-step', type=int, default=1, metavar='K', help='K-step returns in the replay buffer')
    args = ap.parse_args()
    net_arch = tuple(int(w) for w in args.net_arch.split(','))
    kw = dict(kewargs, use_turning=args.turning)
    env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, **kw)
    test_env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, seed=1234, **kw)
    model = DeviceSAC(env, batch=args.batch, net_arch=net_arch, n_step=args.n_step, fused_target=args.fused_target,
                      fused_learner=args.fused_learner)
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
        lq, lpi, la = (float(v) for v in model.losses) if model.losses is not None else (float('nan'),) * 3
        print(f'iter {i}: {args.train_steps * args.envs / dt / 1e6:.2f} M env-steps/s incl. learning  loss_q {lq:.5f} loss_pi {lpi:.5f} '
              f'loss_alpha {la:.5f} ent_coef {float(model.alpha):.4f}  {r}')
    print(f"goal share: {r0['Goal']:.4f} before, {r['Goal']:.4f} after {args.iters} iterations")
    env.close(); test_env.close()


if __name__ == '__main__':
    main()
