#!/usr/bin/env python3
"""TD3 on N vectorised reach_ball envs with a continuous action, everything on the GPU.

The twin-critic companion of ddpg_reach_ball.py for use_continuous_action=True (--turning: the 4-D action), with
stable-baselines3 -- which cannot be installed offline -- replaced by a small plain-torch TD3 with SB3's defaults: an actor
Linear-ReLU-Linear-ReLU-Linear-Tanh, twin critics Q(s, a), target networks for all three with Polyak averaging (tau = 0.005),
target-policy smoothing (target_policy_noise = 0.2, target_noise_clip = 0.5), the delayed policy update (policy_delay = 2: the actor
and every target network move on every second update) and Gaussian action noise.  The replay buffer is
soccer2d_amd.replay.DeviceReplay (n-step transitions on the device, Timeouts bootstrap).

    python examples/td3_reach_ball.py --envs 4096 --iters 10 --train-steps 256 --fused-actor 32 --fused-target --fused-learner

--fused-actor T collects T x N transitions per launch: the engine evaluates the learner's own actor in-kernel with Gaussian
action noise (Engine.rollout_actor with a soccer2d_amd.actor.DeterministicActor); its packed weights are refreshed
with sync() after every optimiser phase.  The first launches act uniformly at random (SB3's learning_starts).  0: one torch
forward and one env.step per step.
--fused-target computes reward + discount * min Q'(s', clamp(mu'(s') + clamp(sigma z, -c, c), -1, 1)) in one launch
(soccer2d_amd.td.Td3Target): the smoothing noise is the kernel's own, drawn afresh on every call.
--fused-learner runs the critics' and the actor's update in HIP (soccer2d_amd.learn.ActorCriticLearner with q2=): step(...,
actor=False) on the updates between two policy updates, and update_targets on the updates that move the actor, as SB3 does.
With --fused-target and --fused-learner together the update is two captured graphs -- sample -> target -> critic step, and sample -> target -> critic step -> actor
step -> update_targets -- replayed in the delay's pattern; the target launch draws fresh noise at every replay.
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
from soccer2d_amd.replay import DeviceReplay  # noqa: E402

kewargs = {
    'change_ball_position': True, 'change_ball_velocity': True,
    'ball_position_x': 0, 'ball_position_y': 0, 'ball_speed': 0, 'ball_direction': 0,
    'min_distance_to_ball': 5.0, 'max_steps': 200,
    'use_continuous_action': True, 'action_space_size': 16, 'use_turning': False,
}


def mlp(n_in, n_out, net_arch=(64, 64), tanh=False):
    layers = []
    for w in net_arch:
        layers += [nn.Linear(n_in, w), nn.ReLU()]
        n_in = w
    layers.append(nn.Linear(n_in, n_out))
    return nn.Sequential(*(layers + ([nn.Tanh()] if tanh else [])))


class DeviceTD3:
    def __init__(self, env, lr=1e-3, gamma=0.99, tau=0.005, buffer=1 << 20, batch=4096, sigma=0.1, policy_delay=2,
                 target_policy_noise=0.2, target_noise_clip=0.5, learning_starts=1, seed=0, n_step=1, fused_target=False,
                 fused_learner=False):
        torch.manual_seed(seed)
        self.env, self.dev = env, env.device
        n_obs, self.n_act = env.observation_space.shape[0], env.action_space.shape[0]
        self.mu = mlp(n_obs, self.n_act, tanh=True).to(self.dev)
        self.q1, self.q2 = mlp(n_obs + self.n_act, 1).to(self.dev), mlp(n_obs + self.n_act, 1).to(self.dev)
        self.mu_target, self.q1_target, self.q2_target = copy.deepcopy(self.mu), copy.deepcopy(self.q1), copy.deepcopy(self.q2)
        self.opt_mu = torch.optim.Adam(self.mu.parameters(), lr=lr)
        self.opt_q = torch.optim.Adam(list(self.q1.parameters()) + list(self.q2.parameters()), lr=lr)
        self.lrn = None
        if fused_learner:                                   # the modules' parameters become views of the learner's buffers
            from soccer2d_amd.learn import ActorCriticLearner
            self.lrn = ActorCriticLearner.from_modules(self.mu, self.q1, self.q2, actor_lr=lr, critic_lr=lr, max_batch=batch,
                                                       device=self.dev)
        self.gamma, self.tau, self.batch, self.sigma, self.policy_delay = gamma, tau, batch, sigma, policy_delay
        self.noise, self.noise_clip = target_policy_noise, target_noise_clip
        self.learning_starts, self.launches = learning_starts, 0
        self.buffer, self.n_step, self.seed, self.fused_target = buffer, n_step, seed, fused_target
        self.stored, self.n_updates, self.graphs = 0, 0, None
        self.loss_q, self.loss_pi = None, None
        self.obs = env.reset().clone()

    @torch.no_grad()
    def predict(self, obs, noise=False):
        a = self.mu(obs)
        if noise:
            a = (a + self.sigma * torch.randn_like(a)).clamp(-1, 1)
        return a

    def replay(self, T):
        """the device replay buffer, made at the first push: it holds at least one record"""
        if not hasattr(self, 'rb'):
            n_obs = self.obs.shape[-1]
            self.rb = DeviceReplay(max(self.buffer, T * self.env.num_envs), n_obs, self.n_act, torch.float32, self.dev,
                                   n_step=self.n_step, gamma=self.gamma, seed=self.seed)
            self.fbatch = self.rb.alloc_batch(self.batch)
            if self.fused_target:
                from soccer2d_amd.td import Td3Target
                self.td = Td3Target(self.mu_target, self.q1_target, self.q2_target, target_policy_noise=self.noise,
                                    target_noise_clip=self.noise_clip, seed=self.seed, device=self.dev)
                self.ftgt = torch.empty((self.batch,), dtype=torch.float32, device=self.dev)
        return self.rb

    def polyak(self):
        with torch.no_grad():
            for net, tgt_net in ((self.mu, self.mu_target), (self.q1, self.q1_target), (self.q2, self.q2_target)):
                for p, pt in zip(net.parameters(), tgt_net.parameters()):
                    pt.mul_(1 - self.tau).add_(p, alpha=self.tau)

    def target(self, b):
        if self.fused_target:                                # one launch: the target actor, the smoothing and both target critics
            return self.td.target(b, out=self.ftgt)
        with torch.no_grad():
            no = b['next_obs']
            a = self.mu_target(no)
            na = (a + (self.noise * torch.randn_like(a)).clamp(-self.noise_clip, self.noise_clip)).clamp(-1, 1)
            x = torch.cat([no, na], 1)
            return b['reward'] + b['discount'] * torch.min(self.q1_target(x), self.q2_target(x)).squeeze(1)

    def update_fused(self, with_actor):
        """--fused-learner: sample -> target -> the critics' step [-> the actor's step -> the Polyak step], the steps in HIP"""
        b = self.rb.sample(self.batch, out=self.fbatch)
        self.lrn.step(b, self.target(b), actor=with_actor)
        if with_actor:
            if self.fused_target:
                self.lrn.update_targets(self.td, self.tau)   # flat buffer to flat buffer; the target modules follow: no sync()
            else:
                self.polyak()

    def capture(self):
        """all three fused: the two updates of the delay's pattern as captured graphs.  One update of each kind runs eagerly on a
        side stream first (they count: update_targets makes its mirror buffers there), then each is captured once."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for with_actor in (False, True):
                self.update_fused(with_actor)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graphs = {}
        for with_actor in (False, True):
            self.graphs[with_actor] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graphs[with_actor]):
                self.update_fused(with_actor)
        return 2

    def optimise(self, n_updates):
        done = 0
        if self.lrn is not None and self.fused_target and self.graphs is None:
            done = self.capture()
            self.n_updates += done
        for _g in range(done, n_updates):
            self.n_updates += 1
            with_actor = self.n_updates % self.policy_delay == 0
            if self.graphs is not None:
                self.graphs[with_actor].replay()             # fresh smoothing noise: the target's draws word counts the replays
                continue
            if self.lrn is not None:
                self.update_fused(with_actor)
                continue
            b = self.rb.sample(self.batch, out=self.fbatch)
            tgt = self.target(b)
            x = torch.cat([b['obs'], b['action']], 1)
            loss_q = nn.functional.mse_loss(self.q1(x).squeeze(1), tgt) + nn.functional.mse_loss(self.q2(x).squeeze(1), tgt)
            self.opt_q.zero_grad(set_to_none=True)
            loss_q.backward()
            self.opt_q.step()
            self.loss_q = loss_q.detach()
            if with_actor:
                loss_pi = -self.q1(torch.cat([b['obs'], self.mu(b['obs'])], 1)).mean()
                self.opt_mu.zero_grad(set_to_none=True)
                loss_pi.backward()
                self.opt_mu.step()
                self.loss_pi = loss_pi.detach()
                self.polyak()
                if self.fused_target:
                    self.td.sync()                           # the next target launch reads the Polyak-averaged weights
        if self.lrn is not None:
            c1, c2 = self.lrn.critics
            self.loss_q, self.loss_pi = c1.stats[0] + c2.stats[0], self.lrn.actor.stats[0]

    def learn(self, vec_steps):
        """one torch forward and one env.step per vector step (the torch-in-the-loop path)"""
        rb = self.replay(1)
        for _ in range(vec_steps):
            if self.launches < self.learning_starts:
                act = torch.rand((self.env.num_envs, self.n_act), device=self.dev) * 2 - 1
            else:
                act = self.predict(self.obs, noise=True)
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
        """The same TD3, experience collected T steps per launch by the fused actor (the learner's own actor in-kernel):
        epsilon = 1 (uniform random actions) for the first learning_starts launches, then the actor with Gaussian noise."""
        from soccer2d_amd.actor import DeterministicActor
        eng = self.env.engine
        if not hasattr(self, 'actor'):
            self.actor = DeterministicActor.from_module(self.mu, device=self.dev, epsilon=1.0, noise_sigma=self.sigma)
            self.rec = eng.alloc_rollout(T, terminal_obs=True)
        rb, rec = self.replay(T), self.rec
        for _ in range((vec_steps + T - 1) // T):
            self.actor.epsilon = 1.0 if self.launches < self.learning_starts else 0.0
            obs0 = eng.obs.clone()                               # the observation the first action is chosen from
            self.env.rollout(T, out=rec, policy=self.actor, terminal_obs=True)
            rb.push(rec, obs0)                                   # T x N n-step transitions, Timeouts bootstrap (one launch)
            self.launches += 1
            self.stored += T * self.env.num_envs
            if self.stored >= self.batch:
                self.optimise(T)
                self.actor.sync()                                # the next launch acts with the new weights
        self.obs = eng.obs.clone()


def test(env, model, vec_steps):
    """deterministic policy (no noise), count info['result'] of finished episodes"""
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
                    help='collect T steps per launch with the in-kernel actor and Gaussian noise (0: one torch forward per step)')
    ap.add_argument('--fused-target', action='store_true',
                    help='the smoothed, clipped double-Q TD targets in one launch (soccer2d_amd.td.Td3Target)')
    ap.add_argument('--fused-learner', action='store_true',
                    help="the critics' and the actor's update in HIP (soccer2d_amd.learn.ActorCriticLearner with q2=)")
    ap.add_argument('--n-step', type=int, default=1, metavar='K', help='K-step returns in the replay buffer')
    args = ap.parse_args()
    kw = dict(kewargs, use_turning=args.turning)
    env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, **kw)
    test_env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, seed=1234, **kw)
    model = DeviceTD3(env, batch=args.batch, n_step=args.n_step, fused_target=args.fused_target, fused_learner=args.fused_learner)
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
        lq, lpi = (float(v) if v is not None else float('nan') for v in (model.loss_q, model.loss_pi))
        print(f'iter {i}: {args.train_steps * args.envs / dt / 1e6:.2f} M env-steps/s incl. learning  loss_q {lq:.5f} loss_pi {lpi:.5f}  '
              f'{r}  ({model.n_updates} updates' + (', captured graphs)' if model.graphs is not None else ')'))
    print(f"goal share: {r0['Goal']:.4f} before, {r['Goal']:.4f} after {args.iters} iterations")
    env.close(); test_env.close()


if __name__ == '__main__':
    main()
