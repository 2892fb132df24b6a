#!/usr/bin/env python3
"""Self-play PPO on the 11v11 engine: one shared policy on all 22 slots, collected inside the cycle kernel.

    python examples/ppo_match_selfplay.py --num-matches 1024 --steps 64 --iterations 20

Per iteration:
  1. ONE launch collects T cycles of N matches: MatchEngine.rollout(T, logp=True, net_index=True, agent_obs='all') with a
     soccer2d_amd.actor.MatchPolicyActor on every slot -- the kernel builds each agent's own-frame row, runs the policy net,
     samples from its categorical distribution and records the row, the index and its log-probability.
  2. The critic stays in torch: one batched forward over the recorded [T, N, 22, 224] rows and the rows after the last cycle.
  3. The per-agent reward is the engine's left-team reward with the sign by side (+ for slots 0..10, - for 11..21); agents are
     flattened into the env axis, [T, N * 22], for soccer2d_amd.gae.gae().  With --shaping goal=1,ball_advance=0.05,... it is
     the cycle kernel's own per-agent shaped reward instead (rollout(..., agent_reward=True)): a launch of a
     random policy holds next to no goals, the shaped terms are dense.  --chaser-only gives the approach and facing terms to
     each team's chaser alone.
  4. Clipped-surrogate epochs whose logp_old is the kernel's record; sync() hands the new weights to the next launch.
  5. Every --eval-every iterations the learner plays a frozen snapshot() of an earlier self on an evaluation engine of half the
     matches (league.play_networks: learner left, snapshot right, both in-kernel), then the snapshot is renewed.

--obs see is the same loop under partial observability: a MatchSeePolicyActor on every slot's 192-word see row,
a [K, 5] table whose rows also turn the neck or change the view width, the vision state stepped in the cycle kernel, the critic on
the recorded see rows, the signed team reward (the see families have no agent reward: --shaping is refused).  No snapshot
opponent exists for see networks, so evaluation plays the deterministic learner's left team against the in-kernel scripted team.

--obs belief is --obs see with a memory: enable_belief(), a MatchSeePolicyActor(obs='belief') on every slot's
192-word belief row -- the cycle kernel builds the see row, takes it into the slot's belief and acts on that -- the critic on the
recorded belief rows (rec['belief']) and belief_peek() for the rows after the last cycle.  --shaping is refused as for see.

--hear (with --obs see or belief) is the talking variant, on the unfused loop: the cycle kernel has no audio yet, so collection
goes cycle by cycle through Soccer2DMatchVecEnv(obs=..., hear=True).  The policy's 224 inputs are [row | hear
row], a second, small Gaussian head produces the 10 payload words, and every agent speaks every cycle; the log-probability of a
step is the categorical one plus the Gaussian one.  No evaluation rounds; --fused-learner and --shaping are refused.

stable-baselines3 cannot be installed offline; the PPO here is a small plain-torch one of the same shape (Tanh MlpPolicy)."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DASH, TURN, KICK, TACKLE = 1.0, 2.0, 3.0, 4.0   # S2D_MCMD_* (include/s2d_match.h)
# 16 actions, (command, a, b): dashes in eight directions, turns, kicks ahead and to the sides, a tackle
ACTION_TABLE = ([[DASH, 100.0, float(d)] for d in (0, 45, 90, 135, 180, -135, -90, -45)] +
                [[TURN, float(m), 0.0] for m in (-60, -15, 15, 60)] +
                [[KICK, 100.0, float(d)] for d in (-45, 0, 45)] + [[TACKLE, 0.0, 0.0]])
NONE = 0.0                                      # S2D_MCMD_NONE
# --obs see, (command, a, b, TurnNeck moment, ChangeView code): the 16 body actions with no view action, then four rows that only
# turn the neck and three that only change the view width (1 narrow, 2 normal, 3 wide)
SEE_ACTION_TABLE = ([row + [0.0, 0.0] for row in ACTION_TABLE] +
                    [[NONE, 0.0, 0.0, float(m), 0.0] for m in (-60, -20, 20, 60)] +
                    [[NONE, 0.0, 0.0, 0.0, float(c)] for c in (1, 2, 3)])


def mlp(n_in, n_out, hidden, act):
    return nn.Sequential(nn.Linear(n_in, hidden), act(), nn.Linear(hidden, hidden), act(), nn.Linear(hidden, n_out))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--num-matches', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=64, help='cycles per launch (T)')
    ap.add_argument('--iterations', type=int, default=10)
    ap.add_argument('--epochs', type=int, default=4)
    ap.add_argument('--minibatches', type=int, default=8)
    ap.add_argument('--hidden', type=int, default=64, choices=(16, 32, 48, 64))
    ap.add_argument('--relu', action='store_true', help='ReLU hidden activations instead of Tanh (SB3\'s MlpPolicy default)')
    ap.add_argument('--lr', type=float, default=3e-4)
    ap.add_argument('--gamma', type=float, default=0.99)
    ap.add_argument('--lam', type=float, default=0.95)
    ap.add_argument('--clip', type=float, default=0.2)
    ap.add_argument('--vf-coef', type=float, default=0.5)
    ap.add_argument('--ent-coef', type=float, default=0.01)
    ap.add_argument('--eval-every', type=int, default=5, help='iterations between evaluation rounds against the snapshot')
    ap.add_argument('--eval-cycles', type=int, default=600)
    ap.add_argument('--shaping', default=None, metavar='TERM=W,...',
                    help='weights of the in-kernel agent reward (goal, ball_advance, approach, facing, kickable, possession); '
                         'default: the signed team reward')
    ap.add_argument('--chaser-only', action='store_true', help='with --shaping: approach and facing for each team\'s chaser only')
    ap.add_argument('--fused-learner', action='store_true',
                    help='the minibatch epochs in HIP (soccer2d_amd.learn.PPOLearner) instead of torch autograd and Adam')
    ap.add_argument('--obs', default='agent', choices=('agent', 'see', 'belief'),
                    help="'see': partial observability -- the policy on see rows (MatchSeePolicyActor), vision stepped in the kernel; "
                         "'belief': the same on belief rows, the belief updated in the kernel too")
    ap.add_argument('--hear', action='store_true',
                    help='the agents talk: [row | hear row] in, a Gaussian head for the 10 payload words; the unfused loop '
                         '(needs --obs see or belief)')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    if args.chaser_only and not args.shaping:
        ap.error('--chaser-only needs --shaping')
    if args.shaping and args.obs in ('see', 'belief'):
        ap.error('--shaping needs --obs agent: the see and belief families of the cycle kernel have no agent reward')
    if args.hear and (args.obs == 'agent' or args.fused_learner or args.shaping):
        ap.error('--hear needs --obs see or belief and goes with neither --fused-learner nor --shaping')
    if args.shaping:
        try:
            args.shaping = {k.strip(): float(v) for k, v in (item.split('=') for item in args.shaping.split(','))}
        except ValueError:
            ap.error('--shaping takes TERM=WEIGHT pairs separated by commas')
    return args


def main_hear(args):
    """the talking variant: collection cycle by cycle through the env, the policy with a second head for what it says"""
    from soccer2d_amd.gae import gae
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    torch.manual_seed(args.seed)
    dev = torch.device(args.device)
    N, T, K, D, W = args.num_matches, args.steps, len(SEE_ACTION_TABLE), 224, 10
    act = nn.ReLU if args.relu else nn.Tanh
    table = torch.tensor(SEE_ACTION_TABLE, device=dev)
    pi, vf = mlp(D, K, args.hidden, act).to(dev), mlp(D, 1, args.hidden, act).to(dev)
    say_mu = mlp(D, W, 16, act).to(dev)                    # the second head: the mean of the payload words
    say_logstd = nn.Parameter(torch.full((W,), -0.5, device=dev))
    opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + list(say_mu.parameters()) + [say_logstd], lr=args.lr)
    env = Soccer2DMatchVecEnv(N, dev, obs=args.obs, hear=True, noise=True, seed=args.seed)

    def dists(o):
        return torch.distributions.Categorical(logits=pi(o)), torch.distributions.Normal(say_mu(o), say_logstd.exp())

    obs = env.reset()
    rows = torch.empty((T, N, 22, D), device=dev)
    idx = torch.empty((T, N, 22), dtype=torch.long, device=dev)
    words = torch.empty((T, N, 22, W), device=dev)
    logp_old, value = torch.empty((T, N, 22), device=dev), torch.empty((T, N, 22), device=dev)
    reward, done = torch.empty((T, N, 22), device=dev), torch.empty((T, N, 22), dtype=torch.uint8, device=dev)
    a = torch.zeros((N, 22, 17), device=dev)
    a[..., 5] = 1.0                                        # said: every agent speaks every cycle; no attention command
    stats = []
    for it in range(args.iterations):
        with torch.no_grad():
            for t in range(T):
                dc, dn = dists(obs)
                k, w = dc.sample(), dn.sample()
                rows[t], idx[t], words[t], value[t] = obs, k, w, vf(obs).squeeze(-1)
                logp_old[t] = dc.log_prob(k) + dn.log_prob(w).sum(-1)
                a[..., :5], a[..., 7:] = table[k], w       # the payload is clamped to [-1, 1] and quantised by the hear step
                obs, r, d, _info = env.step(a)
                reward[t], done[t] = r, d[:, None]
            last_value = vf(obs).squeeze(-1)
        adv, ret = gae(reward.reshape(T, N * 22).contiguous(), done.reshape(T, N * 22).contiguous(),
                       value.reshape(T, N * 22).contiguous(), last_value.reshape(N * 22).contiguous(), args.gamma, args.lam)
        obs_b, act_b, w_b = rows.reshape(-1, D), idx.reshape(-1), words.reshape(-1, W)
        lp_b, adv_b, ret_b = logp_old.reshape(-1), adv.reshape(-1), ret.reshape(-1)
        B = obs_b.shape[0]
        mb = (B + args.minibatches - 1) // args.minibatches
        for _epoch in range(args.epochs):
            perm = torch.randperm(B, device=dev)
            for s in range(0, B, mb):
                i = perm[s:s + mb]
                dc, dn = dists(obs_b[i])
                lp = dc.log_prob(act_b[i]) + dn.log_prob(w_b[i]).sum(-1)
                adv_i = adv_b[i]
                adv_i = (adv_i - adv_i.mean()) / (adv_i.std() + 1e-8)
                ratio = (lp - lp_b[i]).exp()
                pg = -torch.min(ratio * adv_i, ratio.clamp(1 - args.clip, 1 + args.clip) * adv_i).mean()
                v_loss = nn.functional.mse_loss(vf(obs_b[i]).squeeze(-1), ret_b[i])
                ent = dc.entropy().mean() + dn.entropy().sum(-1).mean()
                loss = pg + args.vf_coef * v_loss - args.ent_coef * ent
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        row = dict(iteration=it, policy_loss=float(pg.detach()), value_loss=float(v_loss.detach()), entropy=float(ent.detach()),
                   approx_kl=float((lp_b[i] - lp.detach()).mean()), mean_reward=float(reward[:, :, 0].mean()),
                   heard_share=float(rows[..., 192].mean()))
        stats.append(row)
        print('  '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}' for k, v in row.items()))
    env.close()
    return stats


def main(argv=None):
    args = parse(argv)
    if args.hear:
        return main_hear(args)
    from soccer2d_amd import league
    from soccer2d_amd.actor import MatchPolicyActor, MatchSeePolicyActor
    from soccer2d_amd.gae import gae
    from soccer2d_amd.match import MatchEngine
    torch.manual_seed(args.seed)
    dev = torch.device(args.device)
    belief = args.obs == 'belief'
    see = args.obs == 'see' or belief                      # the see path: 192 words, the [K, 5] table, vision in the kernel
    table = SEE_ACTION_TABLE if see else ACTION_TABLE
    N, T, K, D = args.num_matches, args.steps, len(table), 192 if see else 224
    act = nn.ReLU if args.relu else nn.Tanh
    pi, vf = mlp(D, K, args.hidden, act).to(dev), mlp(D, 1, args.hidden, act).to(dev)
    learner = None
    if args.fused_learner:                                 # torch.optim.Adam's defaults and no gradient clip, as the torch arm
        from soccer2d_amd.learn import PPOLearner
        learner = PPOLearner.from_modules(pi, vf, lr=args.lr, eps=1e-8, max_grad_norm=0.0, clip_range=args.clip, vf_coef=args.vf_coef,
                                          ent_coef=args.ent_coef, max_batch=(T * N * 22 + args.minibatches - 1) // args.minibatches)
    else:
        opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()), lr=args.lr)
    if see:
        actor = MatchSeePolicyActor.from_module(pi, table, device=dev, obs=args.obs)
    else:
        actor = MatchPolicyActor.from_module(pi, table, device=dev)
    eng = MatchEngine(N, dev, noise=True, seed=args.seed)
    if see:
        eng.enable_vision()
    if belief:
        eng.enable_belief('all')
    eng.set_network(actor, 'all')
    if args.shaping:
        eng.set_agent_reward(args.shaping, args.chaser_only)
    eng.reset()
    rec = eng.alloc_rollout(T, with_obs=False)
    eval_eng = MatchEngine(max(1, N // 2), dev, noise=True, seed=args.seed + 1)
    if see:                                                # the learner's left team, greedy, against the scripted right team
        eval_eng.enable_vision()
        if belief:
            eval_eng.enable_belief('left')
        eval_eng.set_controllers({'left': 'external', 'right': 'scripted'})
        eval_actor = actor.snapshot(deterministic=True)
        eval_eng.set_network(eval_actor, 'left')
    frozen = actor.snapshot()
    sign = torch.tensor([1.0] * 11 + [-1.0] * 11, device=dev)
    stats = []
    for it in range(args.iterations):
        if belief:
            eng.rollout(T, out=rec, with_obs=False, logp=True, net_index=True, belief_obs='all')
        elif see:
            eng.rollout(T, out=rec, with_obs=False, logp=True, net_index=True, see_obs='all')
        else:
            eng.rollout(T, out=rec, with_obs=False, logp=True, net_index=True, agent_obs='all', agent_reward=bool(args.shaping))
        rows, idx, logp_old = rec['belief' if belief else 'see' if see else 'agent_obs'], rec['net_index'], rec['logp']
        with torch.no_grad():
            value = vf(rows.reshape(-1, D)).reshape(T, N * 22)
            last_rows = eng.belief_peek() if belief else eng.see('all') if see else eng.agent_observations('all')
            last_value = vf(last_rows.reshape(-1, D)).reshape(N * 22)
        if args.shaping:
            reward = rec['agent_reward'].reshape(T, N * 22)
        else:
            reward = (rec['reward'][:, :, None] * sign).reshape(T, N * 22).contiguous()
        done = rec['done'][:, :, None].expand(T, N, 22).reshape(T, N * 22).contiguous()
        adv, ret = gae(reward, done, value.contiguous(), last_value.contiguous(), args.gamma, args.lam)
        obs_b, act_b = rows.reshape(-1, D), idx.reshape(-1).long()
        lp_b, adv_b, ret_b = logp_old.reshape(-1), adv.reshape(-1), ret.reshape(-1)
        B = obs_b.shape[0]
        mb = (B + args.minibatches - 1) // args.minibatches
        ro = {'obs': obs_b, 'action': idx.reshape(-1).int(), 'logp': lp_b, 'advantage': adv_b, 'return': ret_b}
        for _epoch in range(args.epochs):
            perm = torch.randperm(B, device=dev)
            if learner is not None:                        # a minibatch step per call, the gather by perm in the kernel
                perm = perm.int()
                for s in range(0, B, mb):
                    learner.step(ro, perm[s:s + mb])
                continue
            for s in range(0, B, mb):
                i = perm[s:s + mb]
                d = torch.distributions.Categorical(logits=pi(obs_b[i]))
                lp = d.log_prob(act_b[i])
                a = adv_b[i]
                a = (a - a.mean()) / (a.std() + 1e-8)
                ratio = (lp - lp_b[i]).exp()
                pg = -torch.min(ratio * a, ratio.clamp(1 - args.clip, 1 + args.clip) * a).mean()
                v_loss = nn.functional.mse_loss(vf(obs_b[i]).squeeze(-1), ret_b[i])
                ent = d.entropy().mean()
                loss = pg + args.vf_coef * v_loss - args.ent_coef * ent
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        actor.sync()                                       # the next launch samples from the new policy
        if learner is not None:                            # approx_kl here is SB3's mean((r - 1) - log r), below mean(logp_old - logp)
            row = dict(iteration=it, policy_loss=learner.policy_loss, value_loss=learner.value_loss, entropy=learner.entropy,
                       approx_kl=learner.approx_kl, mean_reward=float(rec['reward'].mean()))
        else:
            row = dict(iteration=it, policy_loss=float(pg.detach()), value_loss=float(v_loss.detach()), entropy=float(ent.detach()),
                       approx_kl=float((lp_b[i] - lp.detach()).mean()), mean_reward=float(rec['reward'].mean()))
        if (it + 1) % args.eval_every == 0 and see:
            eval_actor.params.copy_(actor.params)          # the learner as it is now, on the first maximum
            eval_eng.reset()
            left0, right0 = eval_eng.score_left.clone(), eval_eng.score_right.clone()
            for c in range(0, args.eval_cycles, 64):
                eval_eng.rollout(min(64, args.eval_cycles - c), with_obs=False)
            row.update(eval_goals_learner=int((eval_eng.score_left - left0).sum()),
                       eval_goals_scripted=int((eval_eng.score_right - right0).sum()))
        elif (it + 1) % args.eval_every == 0:
            gl, gr = league.play_networks(eval_eng, actor, frozen, args.eval_cycles)
            row.update(eval_goals_learner=int(gl.sum()), eval_goals_snapshot=int(gr.sum()))
            frozen = actor.snapshot()                      # the next rounds' opponent: the learner as it is now
        stats.append(row)
        print('  '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}' for k, v in row.items()))
    eng.close(); eval_eng.close()
    return stats


if __name__ == '__main__':
    main()
