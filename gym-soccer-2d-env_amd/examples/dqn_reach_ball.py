#!/usr/bin/env python3
"""DQN on N vectorised reach_ball envs, everything on the GPU.

Mirror of the reference's dqn_stable_baselines3.py (same env kwargs :18-31, same train / test
structure :40-71, same Goal/Out/Timeout bookkeeping) with stable-baselines3 -- which cannot be
installed offline -- replaced by a ~100-line DQN that consumes the engine's DEVICE tensors
directly: observations never leave HBM, the replay buffer is a device tensor, one vector step
feeds N transitions.

    python examples/dqn_reach_ball.py --envs 4096 --iters 10 --train-steps 200 --test-steps 250

--fused-actor T collects T x N transitions per launch: the engine evaluates the learner's own network in-kernel
(Engine.rollout_qnet with a soccer2d_amd.actor.QNetActor), epsilon-greedy per env; the actor's packed weights are refreshed
with sync() after every optimiser phase and Timeouts bootstrap from the recorded terminal observations.  The
record goes into a soccer2d_amd.replay.DeviceReplay in one launch and a batch comes out in one; --n-step K stores
K-step returns (targets R + discount * max Q_target(next)).  --fused-target computes those targets in one launch from the target
network (soccer2d_amd.td.QTarget) instead of a chain of torch ops; --double-q reads the target network's value at
the online network's argmax (Double DQN), with or without --fused-target.  --fused-learner (with --fused-actor and --fused-target)
makes every update one call of soccer2d_amd.learn.QLearner -- forward, backward, clip and Adam in HIP -- so an
update is sample -> target -> step (-> update_priorities with --per-alpha).

--episode-stats (with --fused-actor) hands every collected record to soccer2d_amd.episodes.EpisodeStats and prints SB3's
ep_rew_mean / ep_len_mean of the training episodes after each iteration.
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

kewargs = {                      # dqn_stable_baselines3.py:18-31
    'change_ball_position': True, 'change_ball_velocity': True,
    'ball_position_x': 0, 'ball_position_y': 0, 'ball_speed': 0, 'ball_direction': 0,
    'min_distance_to_ball': 5.0, 'max_steps': 200,
    'use_continuous_action': False, 'action_space_size': 16, 'use_turning': False,
}


class QNet(nn.Module):           # SB3 DQN "MlpPolicy" default: two hidden layers of 64
    def __init__(self, n_obs=10, n_act=16, hidden=64, net_arch=None, activation='relu'):
        """net_arch / activation: SB3's policy_kwargs=dict(net_arch=[128, 64, 32, 16], activation_fn=nn.Tanh)"""
        super().__init__()
        act = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}[activation]
        layers, n_in = [], n_obs
        for w in (net_arch or (hidden, hidden)):
            layers += [nn.Linear(n_in, w), act()]
            n_in = w
        self.net = nn.Sequential(*layers, nn.Linear(n_in, n_act))

    def forward(self, x):
        return self.net(x)


class DeviceReplay:
    def __init__(self, capacity, n_obs, device):
        self.cap, self.pos, self.full = capacity, 0, False
        self.obs = torch.empty((capacity, n_obs), device=device)
        self.next_obs = torch.empty((capacity, n_obs), device=device)
        self.act = torch.empty((capacity,), dtype=torch.int64, device=device)
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


class DeviceDQN:
    def __init__(self, env, lr=1e-3, gamma=0.99, buffer=1 << 20, batch=4096, target_every=50, grad_steps=4,
                 eps_start=1.0, eps_end=0.05, eps_decay_steps=300, seed=0, net_arch=None, activation='relu', n_step=1, per_alpha=0.0,
                 per_beta=0.4, fused_target=False, double_q=False, fused_learner=False):
        torch.manual_seed(seed)
        self.buffer, self.n_step, self.seed = buffer, n_step, seed
        self.per_alpha, self.per_beta = per_alpha, per_beta             # alpha 0: the uniform DeviceReplay
        self.fused_target, self.double_q = fused_target, double_q
        self.fused_learner, self.lr = fused_learner, lr
        self.env, self.dev = env, env.device
        self.n_act = env.action_space.n
        self.general = net_arch is not None or activation != 'relu'      # a network only the general fused actor takes
        self.q = QNet(env.observation_space.shape[0], self.n_act, net_arch=net_arch, activation=activation).to(self.dev)
        self.q_target = copy.deepcopy(self.q)
        self.opt = torch.optim.Adam(self.q.parameters(), lr=lr)
        self.rb = DeviceReplay(buffer, env.observation_space.shape[0], self.dev)
        self.gamma, self.batch, self.target_every, self.grad_steps = gamma, batch, target_every, grad_steps
        self.eps_start, self.eps_end, self.eps_decay = eps_start, eps_end, eps_decay_steps
        self.steps = 0
        self.obs = env.reset().clone()
        self.episode_stats = None                                        # --episode-stats: the collected records go through it

    def epsilon(self):
        f = min(1.0, self.steps / self.eps_decay)
        return self.eps_start + f * (self.eps_end - self.eps_start)

    @torch.no_grad()
    def predict(self, obs, eps=0.0):
        greedy = self.q(obs).argmax(dim=1)
        if eps <= 0:
            return greedy
        rnd = torch.randint(0, self.n_act, greedy.shape, device=self.dev)
        return torch.where(torch.rand(greedy.shape, device=self.dev) < eps, rnd, greedy)

    def bootstrap(self, next_obs):
        """the value the target bootstraps from: max_a Q_target(next), or (--double-q) Q_target(next) at the online argmax"""
        qn = self.q_target(next_obs)
        if self.double_q:
            return qn.gather(1, self.q(next_obs).argmax(dim=1, keepdim=True)).squeeze(1)
        return qn.max(dim=1).values

    def learn(self, vec_steps, on_result=None):
        for _ in range(vec_steps):
            act = self.predict(self.obs, self.epsilon())
            nobs, rew, done, info = self.env.step(act)
            res = info['result']
            # bootstrap through time-limit truncation (Timeout) with the terminal observation
            next_obs = torch.where(done.bool().unsqueeze(1), info['terminal_observation'], nobs)
            term = ((res == 1) | (res == 2)).float()          # Goal / Out are true terminations
            self.rb.add(self.obs, act, rew, next_obs, term)
            if on_result is not None:
                on_result(res)
            self.obs = nobs.clone()
            self.steps += 1
            if self.rb.full or self.rb.pos >= self.batch:
                for _g in range(self.grad_steps):
                    o, a, r, no, t = self.rb.sample(self.batch)
                    with torch.no_grad():
                        tgt = r + self.gamma * (1 - t) * self.bootstrap(no)
                    loss = nn.functional.smooth_l1_loss(self.q(o).gather(1, a.unsqueeze(1)).squeeze(1), tgt)
                    self.opt.zero_grad(set_to_none=True)
                    loss.backward()
                    nn.utils.clip_grad_norm_(self.q.parameters(), 10.0)
                    self.opt.step()
            if self.steps % self.target_every == 0:
                self.q_target.load_state_dict(self.q.state_dict())

    def optimise(self, n_updates):
        for _g in range(n_updates):
            o, a, r, no, t = self.rb.sample(self.batch)
            with torch.no_grad():
                tgt = r + self.gamma * (1 - t) * self.bootstrap(no)
            loss = nn.functional.smooth_l1_loss(self.q(o).gather(1, a.unsqueeze(1)).squeeze(1), tgt)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(self.q.parameters(), 10.0)
            self.opt.step()

    def fused_replay(self, T, n_obs):
        """the device replay buffer of the fused path (soccer2d_amd.replay.DeviceReplay, or PrioritizedReplay with --per-alpha),
        made at the first launch: it holds at least one record"""
        from soccer2d_amd.replay import DeviceReplay, PrioritizedReplay
        FusedReplay = PrioritizedReplay if self.per_alpha > 0 else DeviceReplay
        if not hasattr(self, 'frb'):
            self.frb = FusedReplay(max(self.buffer, T * self.env.num_envs), n_obs, 1, torch.int32, self.dev, n_step=self.n_step,
                                   gamma=self.gamma, seed=self.seed)
            self.fbatch, self.stored = self.frb.alloc_batch(self.batch), 0
        return self.frb

    def make_fused_target(self):
        """--fused-target: the target launch's state (soccer2d_amd.td.QTarget) and the tensor it writes, made once"""
        if self.fused_target and not hasattr(self, 'td'):
            from soccer2d_amd.td import QTarget
            self.td = QTarget.from_module(self.q_target, online=self.q if self.double_q else None, device=self.dev)
            self.ftgt = torch.empty((self.batch,), dtype=torch.float32, device=self.dev)
        if self.fused_learner and not hasattr(self, 'learner'):
            from soccer2d_amd.learn import QLearner      # self.q's parameters become views of the learner's flat buffer
            self.learner = QLearner.from_module(self.q, lr=self.lr, max_grad_norm=10.0, loss='huber', max_batch=self.batch, device=self.dev)
            self.fabs = torch.empty((self.batch,), dtype=torch.float32, device=self.dev)

    def optimise_fused(self, n_updates):
        """optimise() on batches of the fused replay buffer: reward is the n-step return, discount gamma^k or 0.  With
        --per-alpha the batch is drawn in proportion to priority, the loss carries the importance weights and the batch's slots
        get (|TD error| + 1e-6) ** alpha as their new priority."""
        for _g in range(n_updates):
            b = self.frb.sample(self.batch, out=self.fbatch)
            if self.fused_learner:                               # sample -> target -> step (-> priorities): one launch chain
                if self.double_q:
                    self.td.online.sync()
                tgt = self.td.target(b, out=self.ftgt)
                if self.per_alpha > 0:
                    self.learner.step(b, tgt, weight=self.frb.weights(b, self.per_beta), td_abs_out=self.fabs)
                    self.frb.update_priorities(b['index'], (self.fabs + 1e-6) ** self.per_alpha)
                else:
                    self.learner.step(b, tgt)
                continue
            if self.fused_target:                                # one launch; the online network's weights as of this step
                if self.double_q:
                    self.td.online.sync()
                tgt = self.td.target(b, out=self.ftgt)
            else:
                with torch.no_grad():
                    tgt = b['reward'] + b['discount'] * self.bootstrap(b['next_obs'])
            q = self.q(b['obs']).gather(1, b['action'].long()).squeeze(1)
            if self.per_alpha > 0:
                loss = (self.frb.weights(b, self.per_beta) * nn.functional.smooth_l1_loss(q, tgt, reduction='none')).mean()
                self.frb.update_priorities(b['index'], ((q.detach() - tgt).abs() + 1e-6) ** self.per_alpha)
            else:
                loss = nn.functional.smooth_l1_loss(q, tgt)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(self.q.parameters(), 10.0)
            self.opt.step()

    def after_fused_launch(self, T):
        """target-network schedule, then grad_steps updates per collected vector step and the actor's new weights"""
        for _t in range(T):
            self.steps += 1
            if self.steps % self.target_every == 0 and self.fused_learner:
                self.learner.update_target(self.td)              # flat buffer to flat buffer; the target module follows
            elif self.steps % self.target_every == 0:
                self.q_target.load_state_dict(self.q.state_dict())
                if self.fused_target:
                    self.td.q_target.sync()                      # the target launch reads the new weights
        self.stored += T * self.env.num_envs
        if self.stored >= self.batch:
            self.optimise_fused(self.grad_steps * T)
            self.actor.sync()                                    # the next launch acts with the new weights

    def learn_fused(self, vec_steps, T, on_result=None):
        """The same DQN, experience collected T steps per launch by the fused actor (the learner's own network in-kernel):
        per launch T x N transitions into the replay buffer, then grad_steps updates per collected vector step, then sync()."""
        from soccer2d_amd.actor import QNetActor
        from soccer2d_amd.mlp_actor import MlpQNetActor
        from soccer2d_amd.wide_actor import WideQNetActor
        if not hasattr(self, 'actor'):
            kw = dict(device=self.dev, epsilon=self.epsilon())
            if not self.general:
                self.actor = QNetActor.from_module(self.q, **kw)
            else:
                try:
                    self.actor = MlpQNetActor.from_module(self.q, **kw)
                except ValueError:      # wider than 128, five layers, Sigmoid, or too large for the LDS: streamed weights
                    self.actor = WideQNetActor.from_module(self.q, **kw)
            print(f'fused actor: {type(self.actor).__name__}')
            self.rec = self.env.engine.alloc_rollout(T, terminal_obs=True)
        self.make_fused_target()
        eng, rec = self.env.engine, self.rec
        rb = self.fused_replay(T, eng.obs.shape[-1])
        for _ in range((vec_steps + T - 1) // T):
            self.actor.epsilon = self.epsilon()
            obs0 = eng.obs.clone()                               # the observation the first action is chosen from
            self.env.rollout(T, out=rec, policy=self.actor, terminal_obs=True)
            rb.push(rec, obs0)                                   # T x N n-step transitions, Timeouts bootstrap (one launch)
            if self.episode_stats is not None:
                self.episode_stats.update_record(rec)
            if on_result is not None:
                on_result(rec['result'].reshape(-1))
            self.after_fused_launch(T)
        self.obs = eng.obs.clone()


def test(env, model, vec_steps):
    """dqn_stable_baselines3.py:44-62 -- greedy policy, count info['result'] of finished episodes."""
    obs = env.reset()
    counts = torch.zeros(4, dtype=torch.int64, device=env.device)
    ret = torch.zeros(env.num_envs, device=env.device)
    ep_ret_sum = torch.zeros((), device=env.device)
    for _ in range(vec_steps):
        act = model.predict(obs) if model is not None else None
        obs, rew, done, info = env.step(act)
        ret += rew
        d = done.bool()
        ep_ret_sum += ret[d].sum()
        ret[d] = 0
        counts += torch.bincount(info['result'].long(), minlength=4)
    c = counts.cpu().tolist()
    n = max(1, c[1] + c[2] + c[3])
    return {'Goal': c[1] / n, 'Out': c[2] / n, 'Timeout': c[3] / n, 'episodes': n,
            'mean_return': float(ep_ret_sum.item()) / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--train-steps', type=int, default=200)
    ap.add_argument('--test-steps', type=int, default=250)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--fused-actor', type=int, default=0, metavar='T',
                    help='collect T steps per launch with the in-kernel epsilon-greedy actor (0: one torch forward per step)')
    ap.add_argument('--net-arch', default=None, metavar='W1,W2,...',
                    help='hidden widths, e.g. 128,64,32,16 (1 to 5 multiples of 4 up to 400; default: 64,64)')
    ap.add_argument('--activation', choices=('relu', 'tanh', 'sigmoid'), default='relu')
    ap.add_argument('--n-step', type=int, default=1, metavar='K', help='with --fused-actor: K-step returns in the replay buffer')
    ap.add_argument('--per-alpha', type=float, default=0.0, metavar='A',
                    help='with --fused-actor: prioritized replay, priority = (|TD error| + 1e-6) ** A (0: uniform sampling)')
    ap.add_argument('--fused-target', action='store_true',
                    help='with --fused-actor: the TD targets in one launch from the target network (soccer2d_amd.td.QTarget)')
    ap.add_argument('--double-q', action='store_true', help="Double DQN: the target network's value at the online network's argmax")
    ap.add_argument('--per-beta', type=float, default=0.4, metavar='B', help='with --per-alpha: the importance-weight exponent')
    ap.add_argument('--fused-learner', action='store_true',
                    help='with --fused-actor and --fused-target: forward, backward, clip and Adam in one call (soccer2d_amd.learn.QLearner)')
    ap.add_argument('--episode-stats', action='store_true',
                    help='with --fused-actor: episode returns / lengths / results of the collected records on the device '
                         '(soccer2d_amd.episodes.EpisodeStats), one more line per iteration')
    args = ap.parse_args()
    if args.episode_stats and args.fused_actor <= 0:
        ap.error('--episode-stats needs --fused-actor T')
    if args.fused_target and args.fused_actor <= 0:
        ap.error('--fused-target needs --fused-actor T')
    if args.fused_learner and not (args.fused_actor > 0 and args.fused_target):
        ap.error('--fused-learner needs --fused-actor T and --fused-target')
    net_arch = [int(w) for w in args.net_arch.split(',')] if args.net_arch else None
    env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, **kewargs)
    test_env = EnvironmentFactory().create_vec('reachball', args.envs, device=args.device, seed=1234, **kewargs)
    model = DeviceDQN(env, net_arch=net_arch, activation=args.activation, n_step=args.n_step, per_alpha=args.per_alpha,
                      per_beta=args.per_beta, fused_target=args.fused_target, double_q=args.double_q, fused_learner=args.fused_learner)
    if args.episode_stats:
        from soccer2d_amd.episodes import EpisodeStats
        model.episode_stats = EpisodeStats(args.envs, device=env.device)      # SB3's window of 100 episodes
    print('random policy:', test(test_env, None, args.test_steps))
    for i in range(args.iters):
        t0 = time.time()
        if args.fused_actor > 0:
            model.learn_fused(args.train_steps, args.fused_actor)
        else:
            model.learn(args.train_steps)
        torch.cuda.synchronize()
        dt = time.time() - t0
        r = test(test_env, model, args.test_steps)
        print(f'iter {i}: {args.train_steps * args.envs / dt / 1e6:.2f} M env-steps/s incl. learning  eps={model.epsilon():.2f}  {r}')
        if model.episode_stats is not None:
            s = model.episode_stats.summary()
            print(f"iter {i}: ep_rew_mean {s['ep_rew_mean']:.4f}  ep_len_mean {s['ep_len_mean']:.2f}  Goal {s['window_goal']:.4f} over the "
                  f"last {s['window']} of {s['episodes']} training episodes")
    env.close(); test_env.close()


if __name__ == '__main__':
    main()
