"""MatchEngine / Soccer2DMatchVecEnv: N lockstep 11v11 matches on one MI355X (include/s2d_match.h).

The reference has no 11v11 task env; what is mirrored is the protobuf schema its agents see
and speak: per-cycle body commands {Dash, Turn, Kick, Tackle} (idl/service.proto:380-402) in,
WorldModel-shaped tensors (ball, teammates/opponents tables, game_mode_type, scores, cycle;
idl/service.proto:144-175, 306-349) out.  Device tensors end to end, zero-copy views of the
engine arena, launches on torch's current stream.  No CPU fallback.
"""
import ctypes as C

import torch

from . import _capi, _capi_match as M

_TD = {'float32': torch.float32, 'int32': torch.int32, 'uint8': torch.uint8, 'int64': torch.int64}
_ITEM = {'float32': 4, 'int32': 4, 'uint8': 1, 'int64': 8}


def make_match_config(seed=0x5EED, env_id_offset=0, auto_reset=True, noise=False, server_params=None,
                      hetero_seed=None, player_type_id=None, player_types=None, **match_params):
    """S2DMatchConfig.  Heterogeneous players: `hetero_seed` draws the 17 non-default PlayerTypes the way
    rcssserver does (s2d_match_generate_player_types); `player_types` = {type id: {field: value}} overrides;
    `player_type_id` = 22 type ids, one per player slot (DoChangePlayerType, idl/service.proto:1393-1433;
    default all 0 = homogeneous)."""
    lib = M.bind(_capi.load_library())
    cfg = M.S2DMatchConfig()
    lib.s2d_match_default_config(C.byref(cfg))
    if server_params or match_params:
        for k, v in (server_params or {}).items():
            if not hasattr(cfg.sp, k):
                raise ValueError(f"unknown ServerParam field {k!r}")
            setattr(cfg.sp, k, float(v))
        for k, v in match_params.items():
            if not hasattr(cfg.mp, k):
                raise ValueError(f"unknown match parameter {k!r}")
            setattr(cfg.mp, k, type(getattr(cfg.mp, k))(v))
        # the default type follows the (possibly overridden) server parameters
        sp, mp = cfg.sp, cfg.mp
        base = dict(player_speed_max=sp.player_speed_max, stamina_inc_max=sp.stamina_inc_max, player_decay=sp.player_decay,
                    inertia_moment=sp.inertia_moment, dash_power_rate=sp.dash_power_rate, player_size=sp.player_size,
                    kickable_margin=mp.kickable_margin, kick_rand=mp.kick_rand, extra_stamina=sp.extra_stamina,
                    effort_max=sp.effort_init, effort_min=sp.effort_min, kick_power_rate=mp.kick_power_rate,
                    catchable_area_l_stretch=1.0)
        for t in range(M.MATCH_PLAYER_TYPES):
            for k, v in base.items():
                setattr(cfg.player_types[t], k, float(v))
    if hetero_seed is not None:
        _capi.check(lib, lib.s2d_match_generate_player_types(C.byref(cfg), None, int(hetero_seed) & 0xFFFFFFFFFFFFFFFF),
                    's2d_match_generate_player_types')
    for t, vals in (player_types or {}).items():
        for k, v in vals.items():
            if k not in M.PLAYER_TYPE_FIELDS:
                raise ValueError(f"unknown PlayerType field {k!r}")
            setattr(cfg.player_types[int(t)], k, float(v))
    if player_type_id is not None:
        ids = [int(v) for v in player_type_id]
        if len(ids) != M.MATCH_PLAYERS:
            raise ValueError("player_type_id needs 22 entries")
        for i, v in enumerate(ids):
            cfg.player_type_id[i] = v
    cfg.seed, cfg.env_id_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_offset)
    cfg.auto_reset, cfg.noise = int(bool(auto_reset)), int(bool(noise))
    _capi.check(lib, lib.s2d_match_validate_config(C.byref(cfg)), 's2d_match_validate_config')
    return cfg


def _is_policy(actor):
    """a MatchPolicyActor (policy slots) rather than a MatchQNetActor"""
    return getattr(actor, 'kind', 'qnet') == 'policy'


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class MatchEngine:
    def __init__(self, num_envs, device='cuda:0', cfg=None, **kwargs):
        self.lib = M.bind(_capi.load_library())
        self.controllers = None                         # no per-slot table (set_controllers)
        self.network, self.network_mask = None, 0       # no network slots (set_network)
        self.opponent_network, self.opponent_mask = None, 0   # no second network (set_opponent_network)
        self.vision = None                              # no vision layer (enable_vision)
        self.belief = None                              # no belief layer (enable_belief)
        self.hearing = None                             # no audio layer (enable_hearing)
        self.agent_reward_weights = None                # no agent reward (set_agent_reward)
        if not torch.cuda.is_available():
            raise RuntimeError("the s2d HIP engine needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.cfg = cfg if cfg is not None else make_match_config(**kwargs)
        self.num_envs = int(num_envs)
        if self.num_envs <= 0:
            raise ValueError("num_envs must be positive")
        nbytes = self.lib.s2d_match_arena_bytes(C.byref(self.cfg), self.num_envs)
        self._raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        shift = (-self._raw.data_ptr()) % 256
        self.arena = self._raw[shift:shift + nbytes]
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.s2d_match_create(C.byref(self.cfg), self.num_envs, self.device.index, self.arena.data_ptr(), nbytes,
                                           self._stream(), C.byref(h))
        _capi.check(self.lib, rc, 's2d_match_create')
        self._h = h
        off = (C.c_int64 * 32)()
        _capi.check(self.lib, self.lib.s2d_match_buffer_offsets(self._h, off, 32), 's2d_match_buffer_offsets')
        n = self.num_envs
        for k, (name, _ct, dt, trail) in enumerate(M.MATCH_BUFFER_FIELDS):
            o = off[k + 1]
            shape = (64, 8) if trail is None else (n,) + tuple(trail)
            count = 1
            for d in shape:
                count *= d
            setattr(self, 'stats_striped' if trail is None else name,
                    self.arena[o:o + count * _ITEM[dt]].view(_TD[dt]).view(shape))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def stats(self):
        """int64[8]: env-steps, goals left/right, matches, kicks, tackles, offsides, ball-outs."""
        return self.stats_striped.sum(dim=0)

    def close(self):
        if getattr(self, '_h', None):
            self.lib.s2d_match_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_controllers(self, spec):
        """Per-slot controllers: `spec` = 22 codes, or {'left': ..., 'right': ...}, with 'external' (0: the caller's actions),
        'random' (1: the in-kernel random policy) or 'scripted' (2: the in-kernel scripted team, include/s2d_match.h).  Rows of
        non-external slots in the caller's actions are never read.  None restores the behaviour without a table."""
        codes = M.controller_codes(spec)
        buf = None if codes is None else (C.c_uint8 * M.MATCH_PLAYERS).from_buffer_copy(codes)
        _capi.check(self.lib, self.lib.s2d_match_set_controllers(self._h, buf), 's2d_match_set_controllers')
        self.controllers = None if codes is None else list(codes)

    def set_network(self, actor, slots='all'):
        """Network slots: `actor` (a MatchQNetActor, or a MatchPolicyActor: policy slots, sampled from the policy's own
        distribution, s2d_match_set_policy_network) chooses the action of every slot in `slots` ('all' | 'left' | 'right' | a
        mask of bits 0..21) inside the cycle kernel, on the slot's agent row (include/s2d_match.h).  It overrides the controller
        table for those slots; the engine keeps the actor's buffers, so sync() / epsilon / set_table() act at the next launch (or
        graph replay).  None clears every network, the opponent network (set_opponent_network) included.

        A see actor (MatchQNetActor(obs='see')) is the see network: it acts on the slot's see row, its table also chooses the
        slot's TurnNeck / ChangeView, and from now on the cycle kernel steps the vision state itself -- do not call vision_step()
        for cycles it runs.  It needs enable_vision() first.  Either kind replaces the other, and the see network also clears
        the opponent network: it stays the engine's only one.  A MatchSeePolicyActor is the see network's stochastic
        counterpart (s2d_match_set_see_policy_network), under the same rules.

        A belief actor (MatchQNetActor(obs='belief') or MatchSeePolicyActor(obs='belief')) is the belief network
        (s2d_match_set_belief_network): a see network that acts on the slot's belief row.  The cycle kernel then also owns the
        belief update of its slots -- it takes each cycle's see row into `belief` before it acts -- so do not call belief_step()
        for cycles it runs.  It needs enable_vision() and enable_belief(...) with the belief's slots containing `slots`.  The
        engine keeps the address of the `belief` tensor, as it does of the vision planes: while a belief network is set, change
        `belief` in place only (belief.copy_(...), belief_step, belief_scan) and never rebind the attribute to another tensor --
        the kernel would go on reading and writing the old one.  enable_belief() is the one call that replaces the tensor, and it
        sets the network again on the new one."""
        if actor is None:
            _capi.check(self.lib, self.lib.s2d_match_set_network(self._h, None), 's2d_match_set_network')
            _capi.check(self.lib, self.lib.s2d_match_set_opponent_network(self._h, None), 's2d_match_set_opponent_network')
            _capi.check(self.lib, self.lib.s2d_match_set_see_network(self._h, None), 's2d_match_set_see_network')
            self.network, self.network_mask = None, 0
            self.opponent_network, self.opponent_mask = None, 0
            return
        mask = M.agent_slot_mask(slots)
        if actor.device != self.device:
            raise ValueError(f"the actor's buffers are on {actor.device}, the engine on {self.device}")
        if getattr(actor, 'obs', 'agent') == 'belief':
            self._need_vision()
            self._need_belief()
            if mask & ~self.belief_mask:
                raise ValueError(f"network slots {mask:#x} are not inside the belief's slots {self.belief_mask:#x} (enable_belief)")
            net = actor.c_struct(mask, self.vision_params, self.vision, self.belief_params, self.belief, self.belief_mask)
            _capi.check(self.lib, self.lib.s2d_match_set_belief_network(self._h, C.byref(net)), 's2d_match_set_belief_network')
            self.opponent_network, self.opponent_mask = None, 0
        elif getattr(actor, 'obs', 'agent') == 'see':
            self._need_vision()
            net = actor.c_struct(mask, self.vision_params, self.vision)
            if _is_policy(actor):
                _capi.check(self.lib, self.lib.s2d_match_set_see_policy_network(self._h, C.byref(net)),
                            's2d_match_set_see_policy_network')
            else:
                _capi.check(self.lib, self.lib.s2d_match_set_see_network(self._h, C.byref(net)), 's2d_match_set_see_network')
            self.opponent_network, self.opponent_mask = None, 0
        else:
            if mask & self.opponent_mask:
                raise ValueError(f"network slots {mask:#x} overlap the opponent network's slots {self.opponent_mask:#x}")
            self._set_role(M.MATCH_ROLE_NETWORK, actor, mask)
        self.network, self.network_mask = actor, mask

    def _set_role(self, role, actor, mask):
        """an agent-row actor into a role of the engine: a policy through s2d_match_set_policy_network, a Q-network through the
        role's own setter"""
        net = actor.c_struct(mask)
        if _is_policy(actor):
            rc, fn = self.lib.s2d_match_set_policy_network(self._h, role, C.byref(net)), 's2d_match_set_policy_network'
        elif role == M.MATCH_ROLE_OPPONENT:
            rc, fn = self.lib.s2d_match_set_opponent_network(self._h, C.byref(net)), 's2d_match_set_opponent_network'
        else:
            rc, fn = self.lib.s2d_match_set_network(self._h, C.byref(net)), 's2d_match_set_network'
        _capi.check(self.lib, rc, fn)

    def set_opponent_network(self, actor, slots='right'):
        """A second, independent network beside set_network's: `actor` (a MatchQNetActor on agent rows or a MatchPolicyActor,
        of either kind whatever set_network's is; typically a frozen ``snapshot()`` of the learner) plays the slots in `slots` on its own weights, epsilon and action table, in the same launch
        (s2d_match_set_opponent_network in include/s2d_match.h).  The two masks must be disjoint; either network may be set
        without the other.  None clears the opponent only.  A see actor is refused: the see network stays single."""
        if actor is None:
            _capi.check(self.lib, self.lib.s2d_match_set_opponent_network(self._h, None), 's2d_match_set_opponent_network')
            self.opponent_network, self.opponent_mask = None, 0
            return
        mask = M.agent_slot_mask(slots)
        if getattr(actor, 'obs', 'agent') in ('see', 'belief'):
            raise ValueError("the opponent network acts on agent rows: a see actor cannot be one (the see network stays single)")
        if actor.device != self.device:
            raise ValueError(f"the actor's buffers are on {actor.device}, the engine on {self.device}")
        if self._see_network_set():
            raise ValueError("a see network is set: it is the engine's only network (set_network(None) first)")
        if mask & self.network_mask:
            raise ValueError(f"opponent slots {mask:#x} overlap the network's slots {self.network_mask:#x}")
        self._set_role(M.MATCH_ROLE_OPPONENT, actor, mask)
        self.opponent_network, self.opponent_mask = actor, mask

    def set_agent_reward(self, weights, chaser_only=False):
        """Agent reward (include/s2d_match.h): the per-agent shaped reward the cycle kernel computes for rollout(...,
        agent_reward=True).  `weights`: a dict by term name (_capi_match.REWARD_TERMS: goal, ball_advance, approach, facing,
        kickable, possession; missing terms are 0) or a sequence of six; None clears.  chaser_only: the individual terms
        approach and facing go to each team's chaser only (the scripted team's rule 5).  The weights live in
        `agent_reward_weights`, a float32 [6] device tensor the kernel reads when it runs: write it in place to anneal (a
        captured graph replays with what it holds).  Refused while a see network is set."""
        if weights is None:
            _capi.check(self.lib, self.lib.s2d_match_set_agent_reward(self._h, None), 's2d_match_set_agent_reward')
            self.agent_reward_weights = None
            return
        w = torch.tensor(M.reward_weights(weights), dtype=torch.float32, device=self.device)
        rw = M.S2DMatchAgentReward(w.data_ptr(), int(bool(chaser_only)))
        _capi.check(self.lib, self.lib.s2d_match_set_agent_reward(self._h, C.byref(rw)), 's2d_match_set_agent_reward')
        self.agent_reward_weights = w

    def _record(self, out, name, T, tail_shape, dtype):
        """out[name], a rollout record [T, *tail_shape]: allocated when absent, else checked (dtype, contiguous, at least T
        steps, the tail)"""
        t = out.get(name)
        if t is None:
            t = out[name] = torch.empty((T,) + tuple(tail_shape), dtype=dtype, device=self.device)
        elif t.dtype != dtype or not t.is_contiguous() or t.shape[0] < T or tuple(t.shape[1:]) != tuple(tail_shape):
            kind, tail = str(dtype).replace('torch.', ''), ','.join(str(d) for d in tail_shape)
            raise ValueError(f"rollout buffer {name!r} must be contiguous {kind} [T>={T},{tail}]")
        return t

    def _see_network_set(self):
        """a see network of any kind is set: a see actor, or a belief actor (a see network on belief rows)"""
        return self.network is not None and getattr(self.network, 'obs', 'agent') in ('see', 'belief')

    def _belief_network_set(self):
        return self.network is not None and getattr(self.network, 'obs', 'agent') == 'belief'

    def _actions(self, actions, T=None):
        if actions is None:
            return None, None
        a = torch.as_tensor(actions, device=self.device).to(torch.float32).contiguous()
        want = (self.num_envs, M.MATCH_PLAYERS, 3) if T is None else (T, self.num_envs, M.MATCH_PLAYERS, 3)
        if tuple(a.shape) != want:
            raise ValueError(f"actions must have shape {want}, got {tuple(a.shape)}")
        return a, C.c_void_p(a.data_ptr())

    def reset(self, mask=None):
        ptr = None
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            if tuple(mask.shape) != (self.num_envs,):
                raise ValueError(f"mask must have shape ({self.num_envs},)")
            ptr = C.c_void_p(mask.data_ptr())
        _capi.check(self.lib, self.lib.s2d_match_reset(self._h, ptr, self._stream()), 's2d_match_reset')
        if self.vision is not None:
            _capi.check(self.lib, self.lib.s2d_match_vision_reset(self._h, C.byref(self.vision), ptr, self._stream()),
                        's2d_match_vision_reset')
        if self.belief is not None:
            _capi.check(self.lib, self.lib.s2d_match_belief_reset(_ptr(self.belief), self.num_envs, self.belief_mask, ptr,
                                                                  self._stream()), 's2d_match_belief_reset')
        if self.hearing is not None:
            _capi.check(self.lib, self.lib.s2d_match_hear_reset(self._h, C.byref(self.hear_params), C.byref(self.hearing), ptr,
                                                                self._stream()), 's2d_match_hear_reset')
        self._keep = mask

    def step(self, actions=None):
        """actions float[N,22,3] = (command, a, b) per player, None = random policy."""
        keep, ptr = self._actions(actions)
        _capi.check(self.lib, self.lib.s2d_match_step(self._h, ptr, self._stream()), 's2d_match_step')
        self._keep = keep
        return self.reward_left, self.done

    def alloc_rollout(self, T, with_obs=True, record_actions=False):
        n, dev = self.num_envs, self.device
        out = dict(obs=torch.empty((T, n, M.MATCH_SLOTS, M.MATCH_OBJ_WORDS), dtype=torch.float32, device=dev) if with_obs else None,
                   reward=torch.empty((T, n), dtype=torch.float32, device=dev),
                   mode=torch.empty((T, n), dtype=torch.int32, device=dev),
                   done=torch.empty((T, n), dtype=torch.uint8, device=dev))
        if record_actions:
            out['actions'] = torch.empty((T, n, M.MATCH_PLAYERS, 3), dtype=torch.float32, device=dev)
        return out

    def rollout(self, n_steps, actions=None, out=None, with_obs=True, record_actions=False, net_index=False, agent_obs=None,
                see_obs=None, view_actions=None, logp=False, agent_reward=False, belief_obs=None):
        """record_actions: out['actions'] float32 [T, N, 22, 3] receives the (command, a, b) each slot's controller chose in
        each cycle, before the engine's own gating (caller slots: the caller's row).  net_index: out['net_index'] int32
        [T, N, 22] receives each network slot's index (-1 for the other slots).  agent_obs = 'all' | 'left' | 'right' | a mask:
        out['agent_obs'] float32 [T, N, k, 224] receives those slots' start-of-cycle agent rows (the learner's obs_t).
        see_obs = 'all' | 'left' | 'right' | a mask: out['see'] float32 [T, N, k, 192] receives those slots' start-of-cycle see
        rows, built in the cycle kernel, which then also steps the vision state (s2d_match_rollout_see): with a see network set,
        beside its slots; without a network, as a record-only see network for this call.  view_actions float32 [T, N, 22, 2] =
        (TurnNeck moment, ChangeView code) of the slots the see network does not play (None: they neither turn nor change).
        logp: out['logp'] float32 [T, N, 22] receives the log-probability of the index each policy slot took (MatchPolicyActor;
        0 for every other slot, Q-network slots included): s2d_match_rollout_policy, with net_index and agent_obs as above.
        With a MatchSeePolicyActor set it is the see policy's record (s2d_match_rollout_see_policy), with net_index, see_obs and
        view_actions as above; a see Q-network has none and logp is refused.
        agent_reward: out['agent_reward'] float32 [T, N, 22] receives every agent's shaped reward of each cycle
        (set_agent_reward first; s2d_match_rollout_reward); it composes with every record above but the see ones.
        belief_obs = 'all' | 'left' | 'right' | a mask (a belief actor set; inside the belief's slots): out['belief'] float32
        [T, N, k, 192] receives the belief rows the network acted on in each cycle -- the belief after that cycle's see row
        (s2d_match_rollout_belief).  It shares its mask with see_obs: giving two different ones raises.  While a belief actor is
        set every launch updates `belief` itself: do not call belief_step() for those cycles."""
        T = int(n_steps)
        if belief_obs is not None:
            if not self._belief_network_set():
                raise ValueError("belief_obs needs a belief network (set_network with a belief actor)")
            if see_obs is not None and M.agent_slot_mask(see_obs) != M.agent_slot_mask(belief_obs):
                raise ValueError("see_obs and belief_obs share one mask: give the same slots for both (or only one of them)")
            if agent_obs is not None or agent_reward:
                raise ValueError("belief_obs excludes agent_obs and agent_reward (the belief network's cycle kernel has neither)")
        keep, ptr = self._actions(actions, T)
        if out is None:
            out = self.alloc_rollout(T, with_obs, record_actions)
        ro = M.S2DMatchRollout()
        for name in ('obs', 'reward', 'mode', 'done'):
            v = out.get(name)
            if v is not None:
                if not v.is_contiguous() or v.shape[0] < T or v.shape[1] != self.num_envs:
                    raise ValueError(f"rollout buffer {name!r} must be contiguous [T>={T},{self.num_envs},...]")
                setattr(ro, name, v.data_ptr())
        n, st = self.num_envs, self._stream()
        rec = self._record(out, 'actions', T, (n, M.MATCH_PLAYERS, 3), torch.float32) if record_actions else None
        va = None
        if agent_reward:
            if see_obs is not None or view_actions is not None or self._see_network_set():
                raise ValueError("agent_reward is not offered with the see network's rollout (its cycle kernel has none)")
            if self.agent_reward_weights is None:
                raise ValueError("agent_reward needs set_agent_reward() first")
            idx = self._record(out, 'net_index', T, (n, M.MATCH_PLAYERS), torch.int32) if net_index else None
            lp = self._record(out, 'logp', T, (n, M.MATCH_PLAYERS), torch.float32) if logp else None
            obs, mask = None, 0
            if agent_obs is not None:
                mask = M.agent_slot_mask(agent_obs)
                obs = self._record(out, 'agent_obs', T, (n, bin(mask).count('1'), M.AGENT_OBS_DIM), torch.float32)
            rwd = self._record(out, 'agent_reward', T, (n, M.MATCH_PLAYERS), torch.float32)
            _capi.check(self.lib, self.lib.s2d_match_rollout_reward(self._h, T, ptr, C.byref(ro), _ptr(rec), _ptr(idx), _ptr(lp), mask,
                                                                     _ptr(obs), _ptr(rwd), st), 's2d_match_rollout_reward')
        elif logp and self._see_network_set() and not _is_policy(self.network):
            raise ValueError("logp is the policy slots' record: the see Q-network has no policy head (MatchSeePolicyActor has)")
        elif (see_obs is not None or view_actions is not None or belief_obs is not None or
              ((net_index or logp) and self._see_network_set())):
            if agent_obs is not None:
                raise ValueError("agent_obs and the see network's rollout exclude each other (one network per engine)")
            va = self._rollout_see(T, ptr, ro, rec, out, net_index, see_obs, view_actions, logp, belief_obs)
        elif net_index or agent_obs is not None or logp:
            idx = self._record(out, 'net_index', T, (n, M.MATCH_PLAYERS), torch.int32) if net_index else None
            obs, mask = None, 0
            if agent_obs is not None:
                mask = M.agent_slot_mask(agent_obs)
                obs = self._record(out, 'agent_obs', T, (n, bin(mask).count('1'), M.AGENT_OBS_DIM), torch.float32)
            if logp:
                lp = self._record(out, 'logp', T, (n, M.MATCH_PLAYERS), torch.float32)
                _capi.check(self.lib, self.lib.s2d_match_rollout_policy(self._h, T, ptr, C.byref(ro), _ptr(rec), _ptr(idx), _ptr(lp),
                                                                         mask, _ptr(obs), st), 's2d_match_rollout_policy')
            else:
                _capi.check(self.lib, self.lib.s2d_match_rollout_net(self._h, T, ptr, C.byref(ro), _ptr(rec), _ptr(idx), mask,
                                                                      _ptr(obs), st), 's2d_match_rollout_net')
        elif rec is not None:
            _capi.check(self.lib, self.lib.s2d_match_rollout_ex(self._h, T, ptr, C.byref(ro), _ptr(rec), st), 's2d_match_rollout_ex')
        else:
            _capi.check(self.lib, self.lib.s2d_match_rollout(self._h, T, ptr, C.byref(ro), st), 's2d_match_rollout')
        self._keep = (keep, out, va)
        return out

    def _rollout_see(self, T, ptr, ro, rec, out, net_index, see_obs, view_actions, logp=False, belief_obs=None):
        """the see network's rollout, the see policy's (logp: with its log-probability record), the belief network's (belief_obs:
        with its row record), or the record-only one; returns the view actions' tensor (for the caller to keep alive)"""
        n, dev = self.num_envs, self.device
        self._need_vision()
        record_only = not self._see_network_set()
        if record_only and (self.network is not None or self.opponent_network is not None):
            raise ValueError("see_obs / view_actions need a see network or no network (the engine has an agent-row network set)")
        idx = self._record(out, 'net_index', T, (n, M.MATCH_PLAYERS), torch.int32) if net_index else None
        lp = self._record(out, 'logp', T, (n, M.MATCH_PLAYERS), torch.float32) if logp else None
        va = None
        if view_actions is not None:
            va = torch.as_tensor(view_actions, device=dev).to(torch.float32).contiguous()
            if tuple(va.shape) != (T, n, M.MATCH_PLAYERS, 2):
                raise ValueError(f"view_actions must have shape ({T}, {n}, {M.MATCH_PLAYERS}, 2), got {tuple(va.shape)}")
        see, mask = None, 0
        if see_obs is not None:
            mask = M.agent_slot_mask(see_obs)
            see = self._record(out, 'see', T, (n, bin(mask).count('1'), M.SEE_DIM), torch.float32)
        if self._belief_network_set():
            bel = None
            if belief_obs is not None:
                mask = M.agent_slot_mask(belief_obs)
                bel = self._record(out, 'belief', T, (n, bin(mask).count('1'), M.BELIEF_DIM), torch.float32)
            if mask & ~self.belief_mask:
                raise ValueError(f"recorded slots {mask:#x} are not inside the belief's slots {self.belief_mask:#x}")
            _capi.check(self.lib, self.lib.s2d_match_rollout_belief(self._h, T, ptr, _ptr(va), C.byref(ro), _ptr(rec), _ptr(idx), _ptr(lp),
                                                                     mask, _ptr(see), _ptr(bel), self._stream()),
                        's2d_match_rollout_belief')
            return va
        if record_only:                                  # no network: the vision state stepped and recorded in-kernel for this call
            net = M.S2DMatchSeeNet()
            net.h1, net.h2, net.n_actions, net.slot_mask = 16, 16, 1, 0
            net.prm, net.vis = self.vision_params, self.vision
            _capi.check(self.lib, self.lib.s2d_match_set_see_network(self._h, C.byref(net)), 's2d_match_set_see_network')
        try:
            if logp:
                _capi.check(self.lib, self.lib.s2d_match_rollout_see_policy(self._h, T, ptr, _ptr(va), C.byref(ro), _ptr(rec), _ptr(idx),
                                                                             _ptr(lp), mask, _ptr(see), self._stream()),
                            's2d_match_rollout_see_policy')
            else:
                _capi.check(self.lib, self.lib.s2d_match_rollout_see(self._h, T, ptr, _ptr(va), C.byref(ro), _ptr(rec), _ptr(idx), mask,
                                                                      _ptr(see), self._stream()), 's2d_match_rollout_see')
        finally:
            if record_only:
                _capi.check(self.lib, self.lib.s2d_match_set_see_network(self._h, None), 's2d_match_set_see_network')
        return va

    def kernel_name(self):
        """which instantiation of the cycle kernel this engine launches (`<stock>`: rules and physics folded into the code)"""
        return self.lib.s2d_match_kernel_name(self._h).decode()

    def relative_tables(self):
        """(dist, angle) float32 [N,22,23]: Player.dist_from_self / angle_from_self (and the ball's, column 22)
        as seen by each of the 22 agents (idl/service.proto:84-85, 155-156)."""
        if getattr(self, '_rel', None) is None:
            shape = (self.num_envs, M.MATCH_PLAYERS, M.MATCH_BALL + 1)
            self._rel = (torch.empty(shape, dtype=torch.float32, device=self.device),
                         torch.empty(shape, dtype=torch.float32, device=self.device))
        d, a = self._rel
        _capi.check(self.lib, self.lib.s2d_match_relative(self._h, d.data_ptr(), a.data_ptr(), self._stream()), 's2d_match_relative')
        return d, a

    def egocentric_tables(self):
        """Per-agent view for policies that act from the player's own frame: dict of device tensors
        dist [N,22,23], bearing [N,22,23] (direction of object j seen from agent p RELATIVE to p's body,
        degrees in (-180, 180]; 0 on the diagonal), teammate [22,23] bool (same side; the ball column is
        False).  Built from the relative-tables kernel (Player.dist_from_self / angle_from_self) and the body
        directions; nothing leaves the device."""
        d, a = self.relative_tables()
        body = self.body[:, :M.MATCH_PLAYERS].unsqueeze(2)
        bearing = a - body
        bearing = torch.where(bearing > 180.0, bearing - 360.0, torch.where(bearing <= -180.0, bearing + 360.0, bearing))
        eye = torch.eye(M.MATCH_PLAYERS, M.MATCH_BALL + 1, dtype=torch.bool, device=self.device)
        bearing = torch.where(eye.unsqueeze(0), torch.zeros_like(bearing), bearing)
        side = torch.arange(M.MATCH_BALL + 1, device=self.device) < 11
        teammate = (side[:M.MATCH_PLAYERS, None] == side[None, :])
        teammate[:, M.MATCH_BALL] = False
        return {'dist': d, 'bearing': bearing, 'teammate': teammate}

    def agent_observations(self, slots='all', out=None):
        """float32 [N, k, 224]: each selected agent's observation in its own team's frame (include/s2d_match.h, "Per-agent
        observations"), rows in ascending slot order.  slots = 'all' (22) | 'left' (slots 0..10) | 'right' (11..21) | a mask of
        bits 0..21.  Computed from the current state by one kernel on torch's current stream; `out` (contiguous, float32, 16-byte
        aligned, [N, k, 224]) is written in place and returned."""
        mask = M.agent_slot_mask(slots)
        shape = (self.num_envs, bin(mask).count('1'), M.AGENT_OBS_DIM)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {self.device}")
        _capi.check(self.lib, self.lib.s2d_match_agent_obs(self._h, mask, C.c_void_p(out.data_ptr()), self._stream()),
                    's2d_match_agent_obs')
        return out

    def enable_vision(self, **params):
        """Switch the vision layer on (include/s2d_match.h, "Vision"): allocates the three state planes -- `neck` float32,
        `view_width` int32, `see_wait` int32, each [N, 24] -- and resets them; from now on reset() resets them with the engine.
        `params`: S2DVisionParams fields over the defaults (view_angle / see_interval: three values, narrow / normal / wide).
        The engine itself does not change: the body step never reads these planes -- unless a see network is set
        (set_network with a see actor), whose cycle kernel steps them.  The engine then holds these planes' addresses and a copy
        of the parameters: a second enable_vision() sets the see network again, on the new planes and parameters."""
        self.vision_params = M.vision_params(self.lib, **params)
        shape = (self.num_envs, M.MATCH_SLOTS)
        self.neck = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.view_width = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.see_wait = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.vision = M.S2DMatchVision(self.neck.data_ptr(), self.view_width.data_ptr(), self.see_wait.data_ptr())
        _capi.check(self.lib, self.lib.s2d_match_vision_reset(self._h, C.byref(self.vision), None, self._stream()),
                    's2d_match_vision_reset')
        if self._see_network_set():                      # the engine kept the old planes' addresses and the old parameters
            self.set_network(self.network, self.network_mask)

    def _need_vision(self):
        if self.vision is None:
            raise RuntimeError("the vision layer is off: call enable_vision() first")

    def vision_step(self, view_actions=None, done=None):
        """One cycle of the vision state; call it once after each body step.  view_actions float32 [N, 22, 2] = (TurnNeck
        moment, ChangeView code 0 keep / 1 narrow / 2 normal / 3 wide) per player, None = nobody turns or changes.  done: None, True
        (the engine's own `done` of the last step) or a uint8 [N] tensor: those matches' vision state is reset instead."""
        self._need_vision()
        a, aptr = None, None
        if view_actions is not None:
            a = torch.as_tensor(view_actions, device=self.device).to(torch.float32).contiguous()
            if tuple(a.shape) != (self.num_envs, M.MATCH_PLAYERS, 2):
                raise ValueError(f"view_actions must have shape ({self.num_envs}, {M.MATCH_PLAYERS}, 2), got {tuple(a.shape)}")
            aptr = C.c_void_p(a.data_ptr())
        d, dptr = None, None
        if done is not None and done is not False:
            d = self.done if done is True else torch.as_tensor(done, device=self.device).to(torch.uint8).contiguous()
            if tuple(d.shape) != (self.num_envs,):
                raise ValueError(f"done must have shape ({self.num_envs},)")
            dptr = C.c_void_p(d.data_ptr())
        _capi.check(self.lib, self.lib.s2d_match_vision_step(self._h, C.byref(self.vision_params), C.byref(self.vision), aptr, dptr,
                                                              self._stream()), 's2d_match_vision_step')
        self._keep_vision = (a, d)

    def see(self, slots='all', out=None):
        """float32 [N, k, 192]: each selected agent's see row in its own team's frame (include/s2d_match.h, "Vision"; the words:
        _capi_match.SEE_FIELDS), rows in ascending slot order; slots and `out` as for agent_observations.  A pure function of
        the current state, the vision planes and the tick."""
        self._need_vision()
        mask = M.agent_slot_mask(slots)
        shape = (self.num_envs, bin(mask).count('1'), M.SEE_DIM)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {self.device}")
        _capi.check(self.lib, self.lib.s2d_match_see(self._h, C.byref(self.vision_params), C.byref(self.vision), mask,
                                                      C.c_void_p(out.data_ptr()), self._stream()), 's2d_match_see')
        return out

    def enable_hearing(self, **params):
        """Switch the audio layer on (include/s2d_match.h, "Hearing"): allocates the hear capacities `cap_our`, `cap_opp` and
        `attention`, int32 [N, 24] each, and the hear rows `hear` float32 [N, 22, 32] (the words: _capi_match.HEAR_FIELDS), and
        resets them; from now on reset() resets them with the engine.  `params`: S2DHearParams fields over the defaults.  The
        engine itself does not change: no kernel of it reads or writes these planes."""
        self.hear_params = M.hear_params(self.lib, **params)
        shape = (self.num_envs, M.MATCH_SLOTS)
        self.cap_our = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.cap_opp = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.attention = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.hear = torch.zeros((self.num_envs, M.MATCH_PLAYERS, M.HEAR_DIM), dtype=torch.float32, device=self.device)
        self.hearing = M.S2DMatchHear(self.cap_our.data_ptr(), self.cap_opp.data_ptr(), self.attention.data_ptr(), self.hear.data_ptr())
        _capi.check(self.lib, self.lib.s2d_match_hear_reset(self._h, C.byref(self.hear_params), C.byref(self.hearing), None,
                                                            self._stream()), 's2d_match_hear_reset')

    def _need_hearing(self):
        if self.hearing is None:
            raise RuntimeError("the audio layer is off: call enable_hearing() first")

    def hear_step(self, say=None, done=None):
        """One cycle of hearing; call it once after each body step, beside vision_step.  say float32 [N, 22, 12] = (said,
        attention command, 10 payload words) per player in raw slot order (_capi_match.SAY_FIELDS), None = nobody speaks or changes
        attention.  done: None, True (the engine's own `done` of the last step) or a uint8 [N] tensor: those matches' hear state
        is reset instead.  The neck plane is passed when the vision layer is on.  Returns `hear` (rewritten in place)."""
        self._need_hearing()
        a, aptr = None, None
        if say is not None:
            a = torch.as_tensor(say, device=self.device).to(torch.float32).contiguous()
            if tuple(a.shape) != (self.num_envs, M.MATCH_PLAYERS, M.SAY_ROW):
                raise ValueError(f"say must have shape ({self.num_envs}, {M.MATCH_PLAYERS}, {M.SAY_ROW}), got {tuple(a.shape)}")
            aptr = C.c_void_p(a.data_ptr())
        d, dptr = None, None
        if done is not None and done is not False:
            d = self.done if done is True else torch.as_tensor(done, device=self.device).to(torch.uint8).contiguous()
            if tuple(d.shape) != (self.num_envs,):
                raise ValueError(f"done must have shape ({self.num_envs},)")
            dptr = C.c_void_p(d.data_ptr())
        nptr = None if self.vision is None else C.c_void_p(self.neck.data_ptr())
        _capi.check(self.lib, self.lib.s2d_match_hear_step(self._h, C.byref(self.hear_params), C.byref(self.hearing), nptr, aptr, dptr,
                                                            self._stream()), 's2d_match_hear_step')
        self._keep_hear = (a, d)
        return self.hear

    def hear_rows(self, slots='all'):
        """float32 [N, k, 32]: the selected agents' hear rows in ascending slot order (slots as for see): a view of `hear` for
        'all' / 'left' / 'right', a gather for any other mask."""
        self._need_hearing()
        mask = M.agent_slot_mask(slots)
        if mask == M.AGENT_SLOT_MASKS['all']:
            return self.hear
        if mask == M.AGENT_SLOT_MASKS['left']:
            return self.hear[:, :11]
        if mask == M.AGENT_SLOT_MASKS['right']:
            return self.hear[:, 11:]
        return self.hear[:, [i for i in range(M.MATCH_PLAYERS) if (mask >> i) & 1]]

    def enable_belief(self, slots='all', **params):
        """Switch the belief layer on (include/s2d_match.h, "Belief"): each selected agent's memory of what it has seen, a row of
        192 words as wide as its see row (the words: _capi_match.BELIEF_FIELDS).  Needs the vision layer.  Allocates `belief`
        float32 [N, k, 192] (rows in ascending slot order; slots as for see) and resets it; from now on reset() resets the
        masked matches' rows.  `params`: S2DBeliefParams fields; ball_decay and player_decay default to the engine's
        ServerParam, view_angle to the vision parameters'.  The layer reads see rows only: the engine does not change -- unless a
        belief network is set (set_network with a belief actor), whose cycle kernel updates `belief`; a second enable_belief()
        then sets that network again on the new buffer and parameters, and refuses slots that no longer contain the network's."""
        self._need_vision()
        if self._belief_network_set() and self.network_mask & ~M.agent_slot_mask(slots):
            raise ValueError(f"a belief network plays slots {self.network_mask:#x}: the belief's slots must contain them")
        params.setdefault('ball_decay', self.cfg.sp.ball_decay)
        params.setdefault('player_decay', self.cfg.sp.player_decay)
        params.setdefault('view_angle', tuple(self.vision_params.view_angle))
        self.belief_params = M.belief_params(self.lib, **params)
        self.belief_mask = M.agent_slot_mask(slots)
        self.belief_slots = slots
        self.belief = torch.empty((self.num_envs, bin(self.belief_mask).count('1'), M.BELIEF_DIM), dtype=torch.float32,
                                  device=self.device)
        _capi.check(self.lib, self.lib.s2d_match_belief_reset(_ptr(self.belief), self.num_envs, self.belief_mask, None,
                                                              self._stream()), 's2d_match_belief_reset')
        if self._belief_network_set():                   # the engine kept the old buffer's address and the old parameters
            self.set_network(self.network, self.network_mask)

    def _need_belief(self):
        if self.belief is None:
            raise RuntimeError("the belief layer is off: call enable_belief() first")

    def _belief_rows(self, t, name, lead, dtype=torch.float32, tail=None):
        """a contiguous device tensor [*lead, N, k, 192] (or [*lead, N] with tail=()) of the belief's shape"""
        tail = tuple(self.belief.shape[1:]) if tail is None else tail
        t = torch.as_tensor(t, device=self.device)
        want = tuple(lead) + (self.num_envs,) + tail
        if t.dtype != dtype:
            if dtype == torch.float32:
                raise ValueError(f"{name} must be float32")
            t = t.to(dtype)
        if tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous tensor of shape {want}, got {tuple(t.shape)}")
        return t

    def belief_step(self, see=None, done=None):
        """One update of the belief with one see row per agent; call it once per cycle, after vision_step.  see: float32
        [N, k, 192] for the belief's slots, None = self.see(slots).  done: None, True (the engine's own `done` of the last step) or
        a uint8 [N] tensor: those matches' beliefs are reset before the row is taken in.  Returns `belief` (updated in place).
        Not for cycles a belief network runs (set_network with a belief actor): its cycle kernel takes each cycle's row in itself."""
        self._need_belief()
        s = self.see(self.belief_slots) if see is None else self._belief_rows(see, 'see', ())
        d = None
        if done is not None and done is not False:
            d = self.done if done is True else self._belief_rows(done, 'done', (), torch.uint8, ())
        rc = self.lib.s2d_match_belief_scan(C.byref(self.belief_params), _ptr(s), _ptr(d), _ptr(self.belief), None, 1,
                                            self.num_envs, self.belief_mask, self._stream())
        _capi.check(self.lib, rc, 's2d_match_belief_scan')
        self._keep_belief = (s, d)
        return self.belief

    def belief_scan(self, see_record, reset=None, out=None):
        """T updates in one launch over a recorded see_record float32 [T, N, k, 192] (a rollout's see record of the belief's
        slots).  reset: uint8 [T, N] or None, a set flag = that match's beliefs are reset before row t is taken in.  A rollout's see
        rows are start-of-cycle rows, so there it is the record's done shifted by one row: reset[0] = 0, reset[t] = done[t - 1];
        for see_record[1:] it is done[:T - 1] as it stands.  out: float32 [T, N, k, 192] or True (allocate it) or
        None: the belief after each row.  `belief` is updated in place to the state after the last row; returns out or belief."""
        self._need_belief()
        s = torch.as_tensor(see_record, device=self.device)
        if s.dim() != 4 or s.shape[0] < 1:
            raise ValueError(f"see_record must have shape (T, {self.num_envs}, {self.belief.shape[1]}, {M.SEE_DIM}) with T >= 1")
        T = int(s.shape[0])
        s = self._belief_rows(s, 'see_record', (T,))
        r = None if reset is None else self._belief_rows(reset, 'reset', (T,), torch.uint8, ())
        if out is True:
            out = torch.empty_like(s)
        elif out is not None:
            out = self._belief_rows(out, 'out', (T,))
        rc = self.lib.s2d_match_belief_scan(C.byref(self.belief_params), _ptr(s), _ptr(r), _ptr(self.belief), _ptr(out), T,
                                            self.num_envs, self.belief_mask, self._stream())
        _capi.check(self.lib, rc, 's2d_match_belief_scan')
        self._keep_belief = (s, r)
        return self.belief if out is None else out

    def belief_peek(self):
        """float32 [N, k, 192]: the belief rows the next launch of a belief network will act on in its first cycle -- `belief`
        after the see rows of the current state, with the engine's done plane as the reset flags -- without changing `belief`.
        One s2d_match_belief_scan of T = 1 on a clone.  What a PPO loop needs for the value of the state after the last cycle."""
        self._need_belief()
        s = self.see(self.belief_slots)
        b = self.belief.clone()
        rc = self.lib.s2d_match_belief_scan(C.byref(self.belief_params), _ptr(s), _ptr(self.done), _ptr(b), None, 1,
                                            self.num_envs, self.belief_mask, self._stream())
        _capi.check(self.lib, rc, 's2d_match_belief_scan')
        self._keep_peek = s
        return b

    def world_model(self):
        """dict proto-path -> device tensor (left team's point of view = absolute coordinates)."""
        P = M.MATCH_PLAYERS
        wm = {'world_model.cycle': self.cycle, 'world_model.stoped_cycle': self.stopped_cycle,
              'world_model.game_mode_type': self.mode, 'world_model.game_mode_side': self.mode_side,
              'world_model.left_team_score': self.score_left, 'world_model.right_team_score': self.score_right,
              'world_model.last_kick_side': self.last_touch_side,
              'world_model.ball.position.x': self.x[:, M.MATCH_BALL], 'world_model.ball.position.y': self.y[:, M.MATCH_BALL],
              'world_model.ball.velocity.x': self.vx[:, M.MATCH_BALL], 'world_model.ball.velocity.y': self.vy[:, M.MATCH_BALL]}
        # the penalty shoot-out (WorldModel.is_penalty_kick_mode, PenaltyKickState: idl/service.proto:336, 130-138), decoded from the
        # set-play word the engine keeps it in (include/s2d_match.h); "our" = the left team
        pen = torch.isin(self.mode, torch.tensor(M.PENALTY_MODES, dtype=self.mode.dtype, device=self.mode.device))   # (27 = IllegalDefense_ is not one)
        w = torch.where(pen, self.set_play_taker, torch.zeros_like(self.set_play_taker))
        wm.update({'world_model.is_penalty_kick_mode': pen,
                   'world_model.penalty_kick_state.on_field_side': torch.where(pen, 2, 0),
                   'world_model.penalty_kick_state.current_taker_side': torch.where(pen & (self.mode != M.GM_PENALTY_ONFIELD), self.mode_side, 0),
                   'world_model.penalty_kick_state.our_taker_counter': (w >> 12) & 15,
                   'world_model.penalty_kick_state.their_taker_counter': (w >> 16) & 15,
                   'world_model.penalty_kick_state.our_score': (w >> 20) & 15,
                   'world_model.penalty_kick_state.their_score': (w >> 24) & 15})
        for team, sl in (('teammates', slice(0, 11)), ('opponents', slice(11, P))):
            for f, t in (('position.x', self.x), ('position.y', self.y), ('velocity.x', self.vx), ('velocity.y', self.vy),
                         ('body_direction', self.body), ('stamina', self.stamina), ('is_tackling', self.tackle_cycles)):
                wm[f'world_model.{team}.{f}'] = t[:, sl]
        return wm


def _is_match_actor(obj):
    from .actor import MatchPolicyActor, MatchQNetActor, MatchSeePolicyActor
    return isinstance(obj, (MatchQNetActor, MatchPolicyActor, MatchSeePolicyActor))


class Soccer2DMatchVecEnv:
    """gym-style surface over MatchEngine for BASELINE.json configs[3] ("11v11 full-match env"):
    ``reset() -> obs``, ``step(actions) -> (obs, reward, done, info)`` with device tensors.

    obs     float32 [N, 23, 5]  (x, y, vx, vy, body) of the 22 players and the ball (row 22), absolute
            coordinates (left team attacks +x); a zero-copy view of the engine's last rollout row.
    actions float32 [N, 22, 3]  (command, a, b) per player, commands of include/s2d_match.h.
    reward  float32 [N]         +1 when the left team scores, -1 when the right team scores
            (zero-sum: the right team's reward is the negative).
    done    uint8 [N]           1 when a match reached TimeOver (auto-restart follows the VecEnv convention).
    info    dict of tensors     game_mode_type, game_mode_side, scores, cycle, nearest player per team.

    opponent = 'random' | 'scripted' | a MatchQNetActor | a MatchPolicyActor: the learner controls the left team only -- actions float32 [N, 11, 3] --
    and the right team is played inside the cycle kernel (the random policy, the scripted team of include/s2d_match.h, or the
    actor's network on each right slot's agent row: a frozen past copy of the learner; a MatchPolicyActor samples from its
    own distribution, or plays its first maximum with deterministic = True).  None: both teams
    come from the caller, as above.

    obs = 'agent': every controlled agent observes in its own team's frame (MatchEngine.agent_observations), so that one policy
    can play either side.  opponent None is self-play: obs float32 [N, 22, 224], actions [N, 22, 3], reward [N, 22] (+reward
    for slots 0..10, its negative for 11..21).  With an in-kernel opponent: obs [N, 11, 224] (the left team only), actions
    [N, 11, 3], reward [N, 11].  The obs tensor is one buffer, rewritten by every reset() / step().

    obs = 'see': partial observability -- every controlled agent gets its see row (MatchEngine.see: view cone, quantised
    distances, identities lost with distance, see timing).  Shapes and rewards as for 'agent' with 192 words per agent, and
    actions float32 [N, 22 or 11, 5] = (command, a, b, TurnNeck moment, ChangeView code).  A step is the body step, then
    vision_step with the engine's done (a restarted match restarts its vision state), then see.  `vision` = a dict of
    S2DVisionParams fields.  The row returned by reset() is not fresh (self and game words only); the first step's is.
    With opponent = a see actor (MatchQNetActor(obs='see') or a MatchSeePolicyActor) the right team plays on its own see rows and turns its necks and
    changes its view as the actor's table says; the cycle kernel then steps the vision state of all 22 players itself (the left
    team's from the caller's TurnNeck / ChangeView words), so a step is one launch plus see.  A see actor needs obs='see' or
    obs='belief'.

    obs = 'belief': partial observability with a memory -- every controlled agent gets its belief row (MatchEngine.belief: the
    layer of include/s2d_match.h, "Belief", over its see rows: identified players in fixed rows, positions predicted while
    unseen, counts of how old each word is).  Actions, shapes and rewards as for 'see'.  A step is the body step, vision_step,
    see, then belief_step with the engine's done (a restarted match forgets); with a see actor as the opponent the one launch,
    then see, then the belief step.  `belief` = a dict of S2DBeliefParams fields.  The obs tensor is the engine's `belief`
    buffer, updated in place; reset(mask) leaves the masked matches' rows unknown.

    hear = True (obs 'see' or 'belief'): the agents talk (MatchEngine.hear_step: the layer of include/s2d_match.h, "Hearing").
    Observations are float32 [N, agents, 224] = [row | hear row] -- the width of an agent row -- and actions [N, agents, 17] =
    the five see words, then the 12 say words (said, attention command, 10 payload words).  A step ends with hear_step on the
    engine's done: what an agent says with its command is in the listeners' next observation.  `hear_params` = a dict of
    S2DHearParams fields.  Not offered while a see actor plays the opponent (that opponent cannot speak yet).

    reward = 'goals' (the default: the rewards above) | a dict by term name | six weights: the shaped per-agent reward the
    cycle kernel computes (MatchEngine.set_agent_reward; chaser_only as there) in the place of the signed team reward, [N, 22]
    or [N, 11], for obs 'agent' and 'see' (not while a see actor plays the opponent; obs='state' has no per-agent reward).
    """

    @staticmethod
    def spaces(opponent=None, obs='state', hear=False):
        """(observation_space, action_space) of an env with this opponent and observation (no engine needed)."""
        import numpy as np
        from .spaces import Box
        if not (opponent in (None, 'random', 'scripted') or _is_match_actor(opponent)):
            raise ValueError(f"opponent must be None, 'random', 'scripted' a MatchQNetActor or a MatchPolicyActor, got {opponent!r}")
        if obs not in ('state', 'agent', 'see', 'belief'):
            raise ValueError(f"obs must be 'state', 'agent', 'see' or 'belief', got {obs!r}")
        agents = 22 if opponent is None else 11
        if hear:
            if obs not in ('see', 'belief'):
                raise ValueError("hear=True needs obs='see' or obs='belief'")
            if _is_match_actor(opponent) and getattr(opponent, 'obs', 'agent') == 'see':
                raise ValueError("hear=True is not offered while a see actor plays the opponent (that opponent cannot speak yet)")
            # [row | hear row]: 192 + 32 words; actions = the five see words, then the 12 say words
            return (Box(low=-1.0e6, high=1.0e6 if obs == 'see' else M.BELIEF_COUNT_LIMIT, shape=(agents, M.SEE_DIM + M.HEAR_DIM),
                        dtype=np.float32),
                    Box(low=-180.0, high=180.0, shape=(agents, 5 + M.SAY_ROW), dtype=np.float32))
        if obs in ('see', 'belief'):               # (a freshly reset belief row holds BELIEF_COUNT_LIMIT in its counts)
            return (Box(low=-1.0e6, high=1.0e6 if obs == 'see' else M.BELIEF_COUNT_LIMIT, shape=(agents, M.SEE_DIM), dtype=np.float32),
                    Box(low=-180.0, high=180.0, shape=(agents, 5), dtype=np.float32))
        if obs == 'agent':
            ospace = Box(low=-1.0e6, high=1.0e6, shape=(agents, M.AGENT_OBS_DIM), dtype=np.float32)
        else:
            ospace = Box(low=-200.0, high=200.0, shape=(23, 5), dtype=np.float32)
        return ospace, Box(low=-180.0, high=180.0, shape=(agents, 3), dtype=np.float32)

    def __init__(self, num_envs, device='cuda:0', opponent=None, obs='state', vision=None, reward='goals', chaser_only=False,
                 belief=None, hear=False, hear_params=None, **kwargs):
        self.observation_space, self.action_space = self.spaces(opponent, obs, hear)
        if hear_params is not None and not hear:
            raise ValueError("hear parameters need hear=True")
        self.hears = bool(hear)
        if _is_match_actor(opponent) and getattr(opponent, 'obs', 'agent') == 'belief':
            raise ValueError("a belief actor is not offered as the in-kernel opponent (the env updates its belief after the cycle, "
                             "the kernel before it); use a see actor with obs='belief'")
        shaped = not (isinstance(reward, str) and reward == 'goals')
        if shaped:
            if isinstance(reward, str):
                raise ValueError(f"reward must be 'goals', a dict by term name or six weights, got {reward!r}")
            if obs == 'state':
                raise ValueError("a shaped reward is per agent: it needs obs='agent', obs='see' or obs='belief'")
            if _is_match_actor(opponent) and getattr(opponent, 'obs', 'agent') == 'see':
                raise ValueError("a shaped reward is not offered while a see network plays the opponent")
            M.reward_weights(reward)                     # (a bad spec fails before the engine exists)
        sees = obs in ('see', 'belief')                  # the agents act under the vision model
        if vision is not None and not sees:
            raise ValueError("vision parameters need obs='see' or obs='belief'")
        if belief is not None and obs != 'belief':
            raise ValueError("belief parameters need obs='belief'")
        self.engine = MatchEngine(num_envs, device, **kwargs)
        self.num_envs, self.device = self.engine.num_envs, self.engine.device
        self.opponent, self.obs_kind = opponent, obs
        self._ro = self.engine.alloc_rollout(1)
        self._see_opponent = _is_match_actor(opponent) and getattr(opponent, 'obs', 'agent') == 'see'
        if self._see_opponent:
            if not sees:
                raise ValueError("a see actor as the opponent needs obs='see' or obs='belief'")
            self.engine.set_controllers({'left': 'external', 'right': 'random'})
            self.engine.enable_vision(**(vision or {}))
            self.engine.set_network(opponent, 'right')
        elif _is_match_actor(opponent):
            # the right team on a frozen network (a past copy of the learner): its slots' controller is the network
            self.engine.set_controllers({'left': 'external', 'right': 'random'})
            self.engine.set_network(opponent, 'right')
        elif opponent is not None:
            self.engine.set_controllers({'left': 'external', 'right': opponent})
        if opponent is not None:
            # the caller's half of the action rows; the right team's rows are never read
            self._act = torch.zeros((1, self.num_envs, M.MATCH_PLAYERS, 3), dtype=torch.float32, device=self.device)
        if sees:
            if not self._see_opponent:
                self.engine.enable_vision(**(vision or {}))
            # the view half of the action rows; an in-kernel opponent's players never turn their necks or change their view
            self._view = torch.zeros((self.num_envs, M.MATCH_PLAYERS, 2), dtype=torch.float32, device=self.device)
        if obs in ('agent', 'see', 'belief'):
            self._slots = 'all' if opponent is None else 'left'
            self._aobs = torch.empty((self.num_envs, self.observation_space.shape[0], M.SEE_DIM if self.hears else
                                      self.observation_space.shape[1]), dtype=torch.float32, device=self.device)
            # reward sign per agent: the left team's reward for slots 0..10, its negative for 11..21
            self._rsign = torch.tensor([1.0] * 11 + ([-1.0] * 11 if opponent is None else []), dtype=torch.float32, device=self.device)
        if obs == 'belief':                              # _aobs takes the see rows, the layer's input; the obs is engine.belief
            self.engine.enable_belief(self._slots, **(belief or {}))
        if self.hears:                                   # the say rows of all 22 players; an in-kernel opponent's never speak
            self.engine.enable_hearing(**(hear_params or {}))
            self._say = torch.zeros((self.num_envs, M.MATCH_PLAYERS, M.SAY_ROW), dtype=torch.float32, device=self.device)
            self._hobs = torch.empty((self.num_envs,) + tuple(self.observation_space.shape), dtype=torch.float32, device=self.device)
        self._shaped = shaped
        if shaped:
            self.engine.set_agent_reward(reward, chaser_only)

    def _obs(self):
        e = self.engine
        if self.hears:                                   # [row | hear row] into one buffer
            row = e.see(self._slots, out=self._aobs) if self.obs_kind == 'see' else e.belief
            self._hobs[..., :M.SEE_DIM] = row
            self._hobs[..., M.SEE_DIM:] = e.hear_rows(self._slots)
            return self._hobs
        if self.obs_kind == 'agent':
            return e.agent_observations(self._slots, out=self._aobs)
        if self.obs_kind == 'see':
            return e.see(self._slots, out=self._aobs)
        if self.obs_kind == 'belief':
            return e.belief
        return torch.stack([e.x[:, :23], e.y[:, :23], e.vx[:, :23], e.vy[:, :23], e.body[:, :23]], dim=2)

    def reset(self, mask=None):
        self.engine.reset(mask)
        return self._obs()

    def _step_see(self, actions):
        agents = 22 if self.opponent is None else 11
        if actions is None:
            raise ValueError(f"with obs={self.obs_kind!r}, step() needs actions [N, {agents}, 5]")
        a = torch.as_tensor(actions, device=self.device).to(torch.float32)
        width = 5 + M.SAY_ROW if self.hears else 5
        if tuple(a.shape) != (self.num_envs, agents, width):
            raise ValueError(f"actions must have shape ({self.num_envs}, {agents}, {width}), got {tuple(a.shape)}")
        self._view[:, :agents] = a[..., 3:5]
        if self.hears:
            self._say[:, :agents] = a[..., 5:]
        return a[..., :3].contiguous()

    def step(self, actions=None):
        if self.obs_kind in ('see', 'belief'):
            actions = self._step_see(actions)
        if self.opponent is None:
            a = None if actions is None else torch.as_tensor(actions, device=self.device).to(torch.float32).reshape(1, self.num_envs, 22, 3)
        else:
            if actions is None:
                raise ValueError("with an in-kernel opponent, step() needs the left team's actions [N, 11, 3]")
            a = torch.as_tensor(actions, device=self.device).to(torch.float32)
            if tuple(a.shape) != (self.num_envs, 11, 3):
                raise ValueError(f"actions must have shape ({self.num_envs}, 11, 3) (the left team), got {tuple(a.shape)}")
            self._act[0, :, :11] = a
            a = self._act
        if self._see_opponent:                            # one launch: the body cycle and the vision step of all 22 players
            self.engine.rollout(1, actions=a, out=self._ro, view_actions=self._view.unsqueeze(0))
        else:
            self.engine.rollout(1, actions=a, out=self._ro, agent_reward=self._shaped)
        e = self.engine
        info = {'game_mode_type': e.mode, 'game_mode_side': e.mode_side, 'left_team_score': e.score_left,
                'right_team_score': e.score_right, 'cycle': e.cycle, 'nearest_left': e.nearest_left, 'nearest_right': e.nearest_right}
        if self.obs_kind in ('see', 'belief') and not self._see_opponent:
            e.vision_step(self._view, done=True)
        if self.obs_kind == 'belief':                     # this cycle's see rows into the memory; a restarted match forgets
            e.belief_step(e.see(self._slots, out=self._aobs), done=True)
        if self.hears:                                    # what was said with this cycle's commands; a restarted match is silent
            e.hear_step(self._say, done=True)
        if self._shaped:                                  # the cycle kernel's per-agent reward, the controlled agents' columns
            return self._obs(), self._ro['agent_reward'][0, :, :self._rsign.numel()], e.done, info
        if self.obs_kind in ('agent', 'see', 'belief'):
            return self._obs(), e.reward_left[:, None] * self._rsign, e.done, info
        return self._ro['obs'][0, :, :23], e.reward_left, e.done, info

    def close(self):
        self.engine.close()
