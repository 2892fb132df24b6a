#!/usr/bin/env python3
"""The reference's python_sample_soccer_env.py experiment on N vectorised GoToCenter envs, everything on the GPU.

Same switches (--continuous --turn --useturn --actor_out_size, :352-359 of the reference script, with its meanings), same
algorithms (DQN on the discrete env; DDPG with ``net_arch=dict(pi=[16, 8], qf=[64, 32, 16, 8])`` otherwise), same Goal / Out /
Timeout bookkeeping as its test(), with stable-baselines3 -- which cannot be installed offline -- replaced by the device-tensor
learners of dqn_reach_ball.py / ddpg_reach_ball.py.

    python examples/go_to_center.py --envs 4096 --iters 10
    python examples/go_to_center.py --continuous --turn --useturn --actor_out_size 4 --fused-actor 32

--fused-actor T collects T x N transitions per launch: the env evaluates the learner's own network in the rollout kernel
(GoToCenterVecEnv.rollout_qnet / rollout_actor with a soccer2d_amd.gtc_actor.GtcQNetActor / GtcDeterministicActor); the actor's
packed weights are refreshed with sync() after every optimiser phase and Timeouts bootstrap from the recorded terminal
observations; the record goes into a soccer2d_amd.replay.DeviceReplay in one launch (--n-step K: K-step returns).
--fused-target computes the TD targets in one launch from the target network(s) (soccer2d_amd.td); --double-q: Double DQN.
--fused-learner (the discrete env, with --fused-actor and --fused-target): every DQN update is one soccer2d_amd.learn.QLearner call.
--fused-learner with --continuous (and --fused-actor): DDPG's critic and actor updates are soccer2d_amd.learn.ActorCriticLearner's.
--net-arch / --activation: the Optuna grids of best_python_sample_soccer_env*.py (1 to 5 widths, multiples of 4 up to 400; relu,
tanh or sigmoid).
"""
import argparse
import copy
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ddpg_reach_ball import DeviceDDPG, mlp  # noqa: E402
from ddpg_reach_ball import test as test_ddpg  # noqa: E402
from dqn_reach_ball import DeviceDQN  # noqa: E402
from dqn_reach_ball import test as test_dqn  # noqa: E402
from soccer2d_amd.gtc import GoToCenterVecEnv  # noqa: E402


class GtcDQN(DeviceDQN):
    def learn_fused(self, vec_steps, T, on_result=None):
        """DeviceDQN.learn_fused on GoToCenterVecEnv.rollout_qnet"""
        from soccer2d_amd.gtc_actor import GtcQNetActor
        if not hasattr(self, 'actor'):
            self.actor = GtcQNetActor.from_module(self.q, device=self.dev, epsilon=self.epsilon())
            print(f'fused actor: {type(self.actor).__name__} {self.actor.hidden} {self.actor.activation}')
            self.rec = None
        self.make_fused_target()
        env = self.env
        rb = self.fused_replay(T, 4)
        for _ in range((vec_steps + T - 1) // T):
            self.actor.epsilon = self.epsilon()
            obs0 = env.obs.clone()                                 # the observation the first action is chosen from
            rec = self.rec = env.rollout_qnet(T, self.actor, terminal_obs=True, out=self.rec)
            rb.push(rec, obs0)                                     # T x N n-step transitions, Timeouts bootstrap (one launch)
            self.after_fused_launch(T)
        self.obs = env.obs.clone()


class GtcDDPG(DeviceDDPG):
    def __init__(self, env, net_arch=None, activation='relu', **kw):
        super().__init__(env, net_arch=net_arch or (16, 8), activation=activation, **kw)      # pi: [16, 8]
        n_obs = env.observation_space.shape[0]
        self.q = mlp(n_obs + self.n_act, 1, net_arch=(64, 32, 16, 8)).to(self.dev)            # qf: [64, 32, 16, 8]
        self.q_target = copy.deepcopy(self.q)
        self.opt_q = torch.optim.Adam(self.q.parameters(), lr=1e-3)

    def learn_fused(self, vec_steps, T):
        """DeviceDDPG.learn_fused on GoToCenterVecEnv.rollout_actor"""
        from soccer2d_amd.gtc_actor import GtcDeterministicActor
        if not hasattr(self, 'actor'):
            self.actor = GtcDeterministicActor.from_module(self.mu, device=self.dev, epsilon=1.0, noise_sigma=self.sigma)
            print(f'fused actor: {type(self.actor).__name__} {self.actor.hidden} {self.actor.activation}')
            self.rec = None
        self.make_fused_target()
        self.make_fused_learner()
        env = self.env
        rb = self.fused_replay(T, 4)
        for _ in range((vec_steps + T - 1) // T):
            self.actor.epsilon = 1.0 if self.launches < self.learning_starts else 0.0
            obs0 = env.obs.clone()
            rec = self.rec = env.rollout_actor(T, self.actor, terminal_obs=True, out=self.rec)
            rb.push(rec, obs0)
            self.after_fused_launch(T)
        self.obs = env.obs.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--train-steps', type=int, default=200)
    ap.add_argument('--test-steps', type=int, default=250)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--continuous', action='store_true', help='Box(-1, 1) dash direction instead of Discrete(16)')
    ap.add_argument('--turn', action='store_true', help='with --continuous: the action row has --actor_out_size entries')
    ap.add_argument('--useturn', action='store_true', help='with --turn: turn angle and the turn / dash choice are actions too')
    ap.add_argument('--actor_out_size', type=int, default=4)
    ap.add_argument('--fused-actor', type=int, default=0, metavar='T',
                    help='collect T steps per launch with the in-kernel actor (0: one torch forward per step)')
    ap.add_argument('--net-arch', default=None, metavar='W1,W2,...',
                    help='hidden widths of the Q-network / the actor (1 to 5 multiples of 4 up to 400; default: 64,64 / 16,8)')
    ap.add_argument('--activation', choices=('relu', 'tanh', 'sigmoid'), default='relu')
    ap.add_argument('--n-step', type=int, default=1, metavar='K', help='with --fused-actor: K-step returns in the replay buffer')
    ap.add_argument('--per-alpha', type=float, default=0.0, metavar='A',
                    help='with --fused-actor: prioritized replay, priority = (|TD error| + 1e-6) ** A (0: uniform sampling)')
    ap.add_argument('--fused-target', action='store_true',
                    help='with --fused-actor: the TD targets in one launch from the target network(s) (soccer2d_amd.td)')
    ap.add_argument('--double-q', action='store_true', help='the discrete env: Double DQN')
    ap.add_argument('--per-beta', type=float, default=0.4, metavar='B', help='with --per-alpha: the importance-weight exponent')
    ap.add_argument('--fused-learner', action='store_true',
                    help='the discrete env, with --fused-actor and --fused-target: forward, backward, clip and Adam in one call; '
                         "--continuous, with --fused-actor: DDPG's critic and actor updates in HIP")
    args = ap.parse_args()
    if args.fused_target and args.fused_actor <= 0:
        ap.error('--fused-target needs --fused-actor T')
    if args.double_q and args.continuous:
        ap.error('--double-q is for the discrete env (DQN)')
    if args.fused_learner and args.continuous and args.fused_actor <= 0:
        ap.error('--fused-learner needs --fused-actor T')
    if args.fused_learner and not args.continuous and not (args.fused_actor > 0 and args.fused_target):
        ap.error('--fused-learner needs --fused-actor T and --fused-target')
    net_arch = [int(w) for w in args.net_arch.split(',')] if args.net_arch else None
    kw = dict(continuous=args.continuous, turn=args.turn, use_turn=args.useturn,
              actor_out_size=args.actor_out_size if (args.turn and args.continuous) else 1)
    env = GoToCenterVecEnv(args.envs, args.device, **kw)
    test_env = GoToCenterVecEnv(args.envs, args.device, seed=1234, **kw)
    learner = dict(net_arch=net_arch, activation=args.activation, n_step=args.n_step, per_alpha=args.per_alpha, per_beta=args.per_beta,
                   fused_target=args.fused_target)
    model, test = (GtcDDPG(env, fused_learner=args.fused_learner, **learner), test_ddpg) if args.continuous else (GtcDQN(env, double_q=args.double_q, fused_learner=args.fused_learner, **learner), test_dqn)
    print('untrained:', test(test_env, model, args.test_steps))
    for i in range(args.iters):
        t0 = time.time()
        if args.fused_actor > 0:
            model.learn_fused(args.train_steps, args.fused_actor)
        else:
            model.learn(args.train_steps)
        torch.cuda.synchronize()
        dt = time.time() - t0
        r = test(test_env, model, args.test_steps)
        print(f'iter {i}: {args.train_steps * args.envs / dt / 1e6:.2f} M env-steps/s incl. learning  '
              f"Goal {r['Goal']:.3f}  Out {r['Out']:.3f}  Timeout {r['Timeout']:.3f}  ({r['episodes']} episodes)")
    env.close(); test_env.close()


if __name__ == '__main__':
    main()
