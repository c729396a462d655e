"""The one-launch rollout of the non-communicating baselines pinned to float64 IN ONE HOP: IC (models.MLP), IRIC-tanh
(models.RNN, rnn_type 'MLP') and IRIC-LSTM (models.RNN, rnn_type 'LSTM') run on kernel stand-ins
(ic3net_amd/models.py:_KernelStandIn) — the NARROW instantiations commnet_forward_kernel<H, PP|TJ, true> of csrc/commnet_fwd.hip
(with h_in for the tanh recurrence) and policy_step_kernel with the communication block off.  Free runs through the Trainer
against oracle.policy_ref (mlp_forward / rnn_forward, numpy float64, the recurrent state carried in float64 from step to step)
driven by the C oracle env on the kernel's own actions, at the project's forward bar of 1e-5: log-probs, value and the state
leaving every step; rewards and the dense obs rows written by the same launch bit for bit; every draw = the oracle's
inverse CDF on the kernel's own log-probs at its Philox position.  Shapes: every narrow instantiation (hid 64 / 128 / 256 on both
envs), the scalar obs-store path (odd dim), a single 32-row MFMA tile, idle rows, last tiles of one env, the training rollout's
record (h_fin / hs / out), short tiles behind full ones, and episode starts inside the launch (auto-reset: a fresh env reads h = 0).

IC3_BASELINE_STEP_ERRORS_OUT=<file>: every case appends its worst figure per quantity and its excused-draw count there as one
JSON line (how profiles/r16/baseline_step_errors.txt was taken)."""
import json
import os

import numpy as np
import pytest
import torch

from test_policy_step_onehop_gpu import _oracle_env

pytestmark = pytest.mark.gpu
TOL = 1e-5          # the project's forward bar (test_policy_step_onehop_gpu.py, test_commnet_step_gpu.py)
EDGE = 1e-6         # a draw may differ from the oracle's only where the float64 CDF of its row has an edge this close to u
MAX_EXCUSED = 1     # ~2e-6 x A per draw, < 2000 draws per case: ~0.02 expected; more than one is a finding, not a seed to change

PP_WORKLOAD = dict(ic="pp_hard_ic", tanh="pp_hard_iric_tanh", lstm="pp_hard_iric")
TJ_BASE = dict(medium="tj_medium", hard="tj_hard", easy="tj_medium")
FAMILY = dict(ic=dict(baseline='mlp', recurrent=False, rnn_type='MLP'),
              tanh=dict(baseline='rnn', recurrent=True, rnn_type='MLP'),
              lstm=dict(baseline='rnn', recurrent=True, rnn_type='LSTM'))


def _build(family, env, E, T, seed, offset, hid):
    """env: ('pp', N, dim, vision) or ('tj', difficulty, N, dim, vision)"""
    import bench
    from ic3net_amd import models, ops
    if env[0] == 'pp':
        _, N, dim, v = env
        tr, a = bench.build_trainer(PP_WORKLOAD[family], E, seed, offset, 0, nagents=N, dim=dim, vision=v, hid_size=hid, max_steps=T)
    else:
        _, diff, N, dim, v = env
        # (cars enter at rate 0.5 so that the few steps played see them)
        tr, a = bench.build_trainer(TJ_BASE[diff], E, seed, offset, 0, commnet=False, ic3net=False, difficulty=diff, nagents=N,
                                    dim=dim, vision=v, hid_size=hid, max_steps=T, add_rate_min=0.5, add_rate_max=0.5,
                                    **FAMILY[family])
    net = tr.policy_net
    assert type(net) is (models.MLP if family == 'ic' else models.RNN), type(net)
    assert a.rnn_type == FAMILY[family]['rnn_type'] and bool(a.recurrent) == FAMILY[family]['recurrent']
    assert len(a.naction_heads) == 1 and len(net.heads) == 1
    raw = tr.env.env
    ok = ops.policy_step_supported(raw, hid) if family == 'lstm' else ops.commnet_step_supported(raw, hid)
    assert ok, "the library refuses %r at hid %d: the case needs the nearest shape it takes" % (env, hid)
    with torch.no_grad():
        net.heads[0].weight.mul_(3.0)                  # peaked action distributions: the draws differ across agents
        if family == 'tanh':
            net.affine2.weight.mul_(2.0)               # the recurrent term is not negligible next to the encoder's
    return tr, a


def _mlp_hidden(p, x):
    """h of models.MLP (models.py:23-34), float64: what rec.h_fin holds"""
    x1 = np.tanh(x @ p['affine1.weight'].T + p['affine1.bias'])
    return np.tanh(x1 @ p['affine2.weight'].T + p['affine2.bias'] + x1)


def _report(case, figures):
    for k in sorted(figures):
        print("baseline-step %s %s %r" % (case, k, figures[k]))
    path = os.environ.get('IC3_BASELINE_STEP_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, **figures), sort_keys=True) + "\n")


def _free_run(case, family, env, hid, E, T, check_envs=None, dense=True, records=False, auto_reset=0, seed=5, offset=300):
    """Plays T lock-step iterations through Trainer.step_episode (the one-launch path) and replays the envs in `check_envs`
    (default: all) through the float64 policy + the oracle env on the kernel's actions.  auto_reset: the step cap of the episodes
    that restart inside the launches (0: off).  Returns the worst figure per quantity."""
    import oracle
    from oracle import philox, policy_ref
    tr, a = _build(family, env, E, T, seed, offset, hid)
    if not dense:
        a.dense_obs = False
    if records:
        tr._records = []                               # the training rollout of the native update
    if auto_reset:
        a.auto_reset = True
    check_envs = list(range(E)) if check_envs is None else list(check_envs)
    N, H = a.nagents, a.hid_size
    params = {k: v.detach().cpu().double().numpy() for k, v in tr.policy_net.state_dict().items()}
    tr.begin_episode(0)
    raw = tr.env.env
    if auto_reset and auto_reset != T:
        raw.set_auto_reset(auto_reset)                 # (the Trainer's own cap is the window: args.max_steps)
    idx = torch.tensor(check_envs, device='cuda')
    pick = lambda x, d=0: x.index_select(d, idx).cpu().numpy()
    rec, left = [], []
    for t in range(T):
        tr.step_episode(t)
        _, action_out, value, _ = tr._step_out[t]
        r = dict(logp=[pick(ao.reshape(E, N, -1)) for ao in action_out], value=pick(value.reshape(E, N)),
                 act=pick(tr._buf['action'][t], 1), rew=pick(tr._buf['reward'][t]), done=pick(tr._buf['done'][t]),
                 obs=pick(raw._obs) if dense else None)
        if family == 'tanh':
            assert tuple(tr._prev_hid.shape) == (E, N, H)
            r['h'] = pick(tr._prev_hid)
            if records:
                left.append(tr._prev_hid.clone())
            if auto_reset:
                # nothing on the Python side rewrites the state between two launches (Trainer._step_body_rnn hands h_out of step t
                # to step t + 1 as it is): the rows of an env that ended here are poisoned — the launch must not read them (`fresh`)
                ended = tr._buf['done'][t].bool()
                tr._prev_hid[ended] = 1e3
        elif family == 'lstm':
            h, c = tr._prev_hid
            r['h'], r['c'] = pick(h.reshape(E, N, H)), pick(c.reshape(E, N, H))
        if records:
            r['out'] = (torch.cat([ao.reshape(E * N, -1) for ao in action_out] + [value.reshape(E * N, 1)], 1)).clone()
        rec.append(r)
    steps = getattr(tr.policy_net, 'mega_steps' if family == 'lstm' else 'commnet_steps', 0)
    assert steps == T, "the one-launch path did not run"
    h_fin = None
    if records:
        er = tr._rec
        assert er is not None and er.n == T and er.out is not None and er.out_n == T
        for t in range(T):
            assert torch.equal(er.out[t], rec[t]['out']), ("rec.out", t)
        if family == 'ic':
            assert er.h_fin is not None and er.h_fin_n == T, "the rollout did not record h (rec.h_fin)"
            h_fin = pick(er.h_fin.reshape(T, E, N, H), 1)
        if family == 'tanh':                           # the entering state of step t IS what left step t - 1
            assert not er.hs[0].any()
            for t in range(1, T):
                assert torch.equal(er.hs[t], left[t - 1].reshape(E * N, H)), ("rec.hs", t)

    tj = a.env_name == 'traffic_junction'
    worst = dict(logp=0.0, value=0.0)
    excused, restarts, followed, draws = 0, 0, 0, 0

    def hold(name, want, got, where):
        err = np.abs(np.asarray(want) - np.asarray(got))
        assert np.isfinite(err).all(), (case, name) + where          # (max() below would let a NaN through)
        worst[name] = max(worst.get(name, 0.0), float(err.max()))

    def zero_state():
        if family == 'tanh':
            return np.zeros((1, N, H))
        return (np.zeros((N, H)), np.zeros((N, H))) if family == 'lstm' else None
    for k, e in enumerate(check_envs):
        gid = offset + e
        o = _oracle_env(a, seed, gid)
        obs = o.reset(0) if tj else o.reset()
        state, tt = zero_state(), 0
        for t in range(T):
            r = rec[t]
            if dense:                                  # the rows of the state acted on, from the same launch
                np.testing.assert_array_equal(r['obs'][k], obs, err_msg="obs rows env %d step %d" % (e, t))
            x = obs[None].astype(np.float64)
            if family == 'ic':
                logp, val = policy_ref.mlp_forward(params, x)
                if h_fin is not None:
                    hold('h_fin', _mlp_hidden(params, x)[0], h_fin[t, k], (e, t))
            elif family == 'tanh':
                logp, val, state = policy_ref.rnn_forward(params, x, state, lstm=False)
                hold('h', state[0], r['h'][k], (e, t))
            else:
                logp, val, state = policy_ref.rnn_forward(params, x, state, lstm=True)
                hold('h', state[0], r['h'][k], (e, t))
                hold('c', state[1], r['c'][k], (e, t))
            hold('logp', logp[0][0], r['logp'][0][k], (e, t))
            hold('value', val.reshape(-1), r['value'][k], (e, t))
            for n in range(N):   # the draw = the oracle's inverse CDF on the kernel's own log-probs at this stream position
                x24 = philox.x24(seed, gid, philox.DOMAIN_SAMPLE, o.episode, tt, n)
                draws += 1
                if oracle.sample_one(r['logp'][0][k, n], x24) != r['act'][0, k, n]:
                    cdf = np.cumsum(np.exp(r['logp'][0][k, n].astype(np.float64)))
                    assert np.abs(cdf - x24 / 2.0 ** 24).min() < EDGE, ("draw", case, e, t, n)
                    excused += 1
            obs, orew, od = o.step(r['act'][0, k])
            tt += 1
            np.testing.assert_array_equal(r['rew'][k], np.asarray(orew).astype(np.float32), err_msg="reward env %d step %d" % (e, t))
            if auto_reset:
                end = bool(od) or tt == auto_reset
                assert bool(r['done'][k]) == end, ("done", case, e, t)
                if end:                                # the next episode of this env starts inside the next launch, from h = 0
                    restarts += 1
                    followed += t + 1 < T              # ... and that launch is one of this window's
                    obs = o.reset(0) if tj else o.reset()
                    state, tt = zero_state(), 0
            elif od:
                break
    _report(case, dict(worst, excused=excused, draws=draws, restarts=restarts, restarts_followed=followed))
    bad = {q: v for q, v in worst.items() if not v < TOL}
    assert not bad, (case, bad)
    assert excused <= MAX_EXCUSED, (case, excused)
    return dict(worst, restarts=restarts, restarts_followed=followed)


PP_A = ('pp', 10, 20, 1)      # 20 rows in a tile of 2 envs with obs rows: one 32-row MFMA tile; the last tile holds one env
PP_C = ('pp', 3, 5, 0)        # odd dim: vocab 29, the scalar obs-store path; one idle row per 21-env tile
PP_D = ('pp', 32, 12, 2)      # at most 2 envs per tile; hid 256: B fragments from L2, one workgroup per CU
PP_E = ('pp', 1, 5, 1)        # a single agent, up to 64 envs per tile
TJ_F = ('tj', 'medium', 10, 14, 1)
TJ_G = ('tj', 'easy', 5, 6, 1)
TJ_H = ('tj', 'hard', 20, 18, 1)      # 3 envs per tile
SMALL = {
    # id: (env, hid, E, T, dense obs rows, the training rollout's record)
    "a": (PP_A, 128, 13, 12, True, False),
    "b": (PP_A, 128, 13, 12, False, True),     # plan_commnet_tiles: 6 envs per tile (both MFMA row tiles), a last tile of one env
    "c": (PP_C, 64, 50, 8, True, False),
    "d": (PP_D, 256, 5, 4, True, False),
    "e": (PP_E, 64, 70, 5, True, False),
    "f": (TJ_F, 128, 13, 14, True, False),     # the narrow TJ launch: zero-filled rows + patches
    "g": (TJ_G, 256, 30, 10, True, False),
    "h": (TJ_H, 64, 7, 14, True, False),
}


@pytest.mark.parametrize("family", ["ic", "tanh"])
@pytest.mark.parametrize("shape", sorted(SMALL))
def test_baseline_step_vs_fp64_reference_policy(shape, family):
    """Every narrow instantiation of commnet_forward_kernel at small shapes, all envs checked.  (b) is the training rollout: no
    obs rows, the episode record armed — IC: rec.h_fin against the float64 h; tanh: rec.hs[t] = the state that left step t - 1,
    bit for bit; both: rec.out[t] = the step's own rows, bit for bit."""
    env, hid, E, T, dense, records = SMALL[shape]
    _free_run("%s-%s" % (shape, family), family, env, hid, E, T, dense=dense, records=records)


@pytest.mark.parametrize("shape", ["a", "c", "g"])
def test_iric_lstm_stand_in_vs_fp64_reference_policy(shape):
    """IRIC-LSTM runs policy_step_kernel (pinned by test_policy_step_onehop_gpu.py) on a stand-in: parameter copies, C zero, no gate
    head — at hid 128 (PP), hid 64 (PP, odd dim) and hid 256 (TJ)."""
    env, hid, E, T, dense, records = SMALL[shape]
    _free_run("%s-lstm" % shape, "lstm", env, hid, E, T, dense=dense, records=records)


def _tile_plan(E, N, cus):
    """plan_commnet_tiles (csrc/commnet_fwd.hip) -> (full tiles, envs per full tile, short tiles, envs per short tile)"""
    ept, epts = 64 // N, 32 // N
    n_all = -(-E // ept)
    if epts < 1:
        return n_all, ept, 0, ept
    n_full = (E // ept) // cus * cus
    if n_full < cus:
        return n_all, ept, 0, ept
    n_short = -(-(E - n_full * ept) // epts)
    if n_full // cus + 0.5 * (-(-n_short // cus)) < float(-(-n_all // cus)) - 1e-9:
        return n_full, ept, n_short, epts
    return n_all, ept, 0, ept


@pytest.mark.parametrize("family,env,extra", [("tanh", TJ_H, 5), ("ic", PP_A, 7)], ids=["tanh-tj_hard", "ic-pp_hard"])
def test_baseline_step_on_short_tiles(family, env, extra):
    """plan_commnet_tiles gives short tiles (one 32-row MFMA tile) only behind at least one full round of tiles: one full tile per
    CU and `extra` envs more — on 256 CUs E = 773 (TJ-hard, N = 20: 256 tiles of 3 envs + 5 short tiles of one) and E = 1543 (PP-hard
    without obs rows, N = 10: 256 tiles of 6 envs + 3 short tiles of 3).  Envs of the first and the last full tile and of the first,
    a middle and the last short tile."""
    N = env[-3]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    E = cus * (64 // N) + extra
    n_full, ept, n_short, epts = _tile_plan(E, N, cus)
    assert n_short > 0 and n_full == cus, ("the case does not reach short tiles on %d CUs" % cus, E, n_full, n_short)
    first_short = n_full * ept
    envs = [0, ept - 1, first_short - ept, first_short - 1, first_short, first_short + (n_short // 2) * epts, E - 1]
    assert sorted(set(envs)) == envs and envs[-1] >= first_short + (n_short - 1) * epts
    # (PP: with obs rows the narrow launch takes plan_store_bound_ept's tiles instead — test_narrow_launch_does_not_depend_on_its_tile_plan)
    _free_run("short-%s-%s" % (family, env[0]), family, env, 128, E, 3, check_envs=envs, dense=env[0] == 'tj')


@pytest.mark.parametrize("cap", [12, 4], ids=["cap12", "cap4"])
@pytest.mark.parametrize("family", ["tanh", "ic", "lstm"])
def test_baseline_step_on_an_auto_reset_handle(family, cap):
    """An env that finishes (Predator-Prey 'mixed': every predator on the prey; or the step cap) restarts inside the launch: the
    float64 replay plays consecutive oracle episodes per env and starts each from a zero recurrent state.  The tanh family's h_in
    rows of the envs that ended are overwritten with 1e3 in front of the next launch: a fresh env reads h = 0, not its rows.
    cap12: the Trainer's own mode, the step cap is the window — the cap ends the episodes at the window's last step, only an
    episode that ends early starts another one inside it (a handful of the 24 envs: `restarts_followed` in the figures).  cap4: the handle's cap set to 4
    steps, so EVERY env starts two episodes inside the window (steps 4 and 8) and plays them on."""
    E, T = 24, 12
    got = _free_run("autoreset-%s-cap%d" % (family, cap), family, ('pp', 2, 3, 1), 64, E, T, auto_reset=cap, seed=7, offset=500)
    assert got['restarts'] > E // 4, "no episode ended: the test would not see a restart"
    if cap < T:
        assert got['restarts_followed'] >= 2 * E, "every env starts an episode at steps 4 and 8 of the window"
