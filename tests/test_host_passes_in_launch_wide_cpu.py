"""CPU: `ic3_policy_step` with `ic3_policy.npasses` = 2..4 at hid_size 256 — every communication pass of the step inside ONE launch
(policy_step_kernel<256, PP | TJ, 1, 1, 0, 0>) — on the host build (tests/host: policy_step.hip unmodified behind the C ABI,
`device = -1`), against one launch per pass of the same library (inner_pass calls for passes 0 .. P-2, the ordinary call for the last).

Two handles are created from one seed and free-run T steps each (the masks of step t - 1 handed over).  Everything a step writes
must be the SAME BITS either way: out, action, the dense observation rows, reward, done, alive, is_completed, h, c.  The npasses run
of the Predator-Prey case is then replayed env by env through oracle.policy_ref (float64, comm_passes = 2) on the C oracle's env at the
project's 1e-5 (TOL of test_host_policy_step_cpu.py).

512 emulated lanes per tile and K = 512: a pass of a tile costs a second or two here, so T is 2..4 and only the two cases that need a
full tile and a remainder tile have them (about three seconds per pass of a full tile)."""
import ctypes as C
import functools

import numpy as np
import pytest

from host_abi_util import HostPolicy, check, p
from test_host_policy_step_cpu import TOL, make_oracle, make_params
from test_host_policy_window_cpu import _env

H = 256
CASES = {
    # 21 envs per 64-row tile: a full tile and a half-tile remainder; the gate chain (the last head's draws are the next step's gate)
    'pp_p2': dict(env='pp', N=3, dim=5, vision=1, heads=[5, 2], hard_attn=True, E=23, T=2, passes=2),
    # cars enter and leave: the alive slice of step t - 1 is step t's mask; every pass shares C_modules[0]; 12 envs per tile
    'tj_easy_p3_shared': dict(env='tj', N=5, dim=6, vision=1, difficulty='easy', heads=[2, 2], hard_attn=True, rate=0.3, E=14, T=2,
                              passes=3, shared=True),
    # auto-reset: episodes of 3 steps restart inside the run (zero state in pass 0 only); comm_action_one (a gate of ones)
    'pp_auto_p2': dict(env='pp', N=3, dim=5, vision=1, heads=[5, 2], hard_attn=False, ones=True, auto=3, E=4, T=4, passes=2),
    # the pass limit; no gate at all
    'pp_p4': dict(env='pp', N=2, dim=3, vision=1, heads=[5], hard_attn=False, E=3, T=2, passes=4),
}
FIELDS = ('out', 'action', 'obs', 'reward', 'done', 'alive', 'comp', 'h', 'c')


def _params(w, obs_dim, seed):
    P = make_params(obs_dim, H, w['heads'], seed=seed, comm_passes=w['passes'])
    if w.get('shared'):                                         # share_weights: every pass runs C_modules[0]
        for i in range(1, w['passes']):
            P['C_modules.%d.weight' % i] = P['C_modules.0.weight']
            P['C_modules.%d.bias' % i] = P['C_modules.0.bias']
    return P


SEED, OFFSET = 7, 40


@functools.lru_cache(maxsize=None)
def _play(name, one_launch):
    """T free-running steps from the zero state; per step a dict of FIELDS (copies) + the snapshot of the state entering it."""
    w = CASES[name]
    env = _env(w, SEED, OFFSET)
    E, N, P_ = w['E'], w['N'], w['passes']
    P = _params(w, env.obs_dim, SEED + 1)
    if one_launch:
        pol = HostPolicy(env, P, H, w['heads'], gate_split=True, passes=P_)
    else:
        pols = [HostPolicy(env, P, H, w['heads'], gate_split=True, pass_index=i, inner=(i + 1 < P_)) for i in range(P_)]
    h = np.zeros((E * N, H), np.float32)
    c = np.zeros((E * N, H), np.float32)
    alive_in = None
    gate = np.zeros((E, N), np.int32) if w['hard_attn'] else np.ones((E, N), np.int32) if w.get('ones') else None
    rec = []
    for t in range(w['T']):
        snap = env.snapshot()
        if one_launch:
            res = pol.step(env, h, c, alive_in, gate)
        else:
            for q in pols[:-1]:
                q.inner_pass(env, h, c, alive_in, gate)
            res = pols[-1].step(env, h, c, alive_in, gate)
        out, act, obs, rew, done, alive, comp = res
        rec.append(dict(out=out.copy(), action=act.copy(), obs=obs.copy(), reward=rew.copy(), done=done.copy(), alive=alive.copy(),
                        comp=comp.copy(), h=h.copy(), c=c.copy(), snap=np.array(snap).copy()))
        if w['env'] == 'tj':
            alive_in = alive
        if w['hard_attn']:
            gate = np.ascontiguousarray(act[len(w['heads']) - 1])
    t_off, t_cnt = env._field('t')
    env.close()
    return rec, slice(t_off, t_off + t_cnt)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_passes_in_one_launch_write_the_bits_of_one_launch_per_pass(name):
    w = CASES[name]
    (ref, tf), (one, _) = _play(name, False), _play(name, True)
    for t, (a, b) in enumerate(zip(ref, one)):
        for key in FIELDS:
            np.testing.assert_array_equal(b[key], a[key], err_msg="%s step %d: %s" % (name, t, key))
        assert np.isfinite(a['out']).all() and np.isfinite(a['h']).all() and np.isfinite(a['c']).all() and (a['action'] >= 0).all()
        assert np.isfinite(a['obs']).all(), "the last pass assembles the dense observation rows"
    assert any((a['obs'] != 0).any() for a in ref)
    # the condition the case exists for, on the per-pass side's draws
    if name == 'pp_p2':
        assert w['E'] > 64 // w['N'] and (w['E'] % (64 // w['N'])) * w['N'] <= 32, "a full tile and a half-tile remainder"
        gate = np.stack([r['action'][-1] for r in ref])
        assert (gate == 0).any() and (gate == 1).any(), "the last head's draws do not carry both gate values"
    if name == 'tj_easy_p3_shared':
        assert w['E'] > 64 // w['N'], "a full tile and a remainder tile"
        alive = np.stack([r['alive'] for r in ref])
        assert (alive[1:] != alive[:-1]).any() and (alive == 0).any() and (alive == 1).any(), "no car's alive flag changes"
    if name == 'pp_auto_p2':
        tstep = np.stack([r['snap'][tf] for r in ref])
        assert (tstep[1:] == 0).any(), "no env restarts inside the run"
        t0 = int(np.argwhere((tstep[1:] == 0).any(1))[0, 0]) + 1
        assert (ref[t0 - 1]['h'] != 0).any(), "the restarting env's state was zero anyway"


def test_the_launch_stays_within_1e_5_of_the_float64_policy_with_two_passes():
    """The npasses run of the Predator-Prey case, env by env: oracle.policy_ref.forward(comm_passes = 2) in float64 on the C oracle's
    env, driven by the launch's own actions."""
    from oracle import policy_ref
    w = CASES['pp_p2']
    rec, _ = _play('pp_p2', True)
    E, N, heads = w['E'], w['N'], w['heads']
    P = _params(w, rec[0]['obs'].shape[-1], SEED + 1)
    worst = 0.0
    for e in range(E):
        o = make_oracle(w, SEED, OFFSET + e)
        obs = o.reset()
        hc = (np.zeros((N, H)), np.zeros((N, H)))
        g = np.zeros(N)
        for t, r in enumerate(rec):
            np.testing.assert_array_equal(r['obs'][e], obs, err_msg="obs rows env %d step %d" % (e, t))
            logp, val, hc = policy_ref.forward(P, obs[None].astype(np.float64), hc, None, g, recurrent=True, comm_passes=2,
                                               hard_attn=True, nheads=2)
            o3 = r['out'].reshape(E, N, -1)[e]
            off = 0
            for hd, A in enumerate(heads):
                worst = max(worst, np.abs(logp[hd][0] - o3[:, off:off + A]).max())
                off += A
            worst = max(worst, np.abs(val.reshape(-1) - o3[:, off]).max())
            worst = max(worst, np.abs(hc[0] - r['h'].reshape(E, N, H)[e]).max(), np.abs(hc[1] - r['c'].reshape(E, N, H)[e]).max())
            obs, orew, _ = o.step(r['action'][0, e])
            np.testing.assert_array_equal(r['reward'][e], np.asarray(orew).astype(np.float32))
            g = r['action'][len(heads) - 1, e].astype(np.float64)
    print("worst |launch - float64| over %d envs x %d steps: %.3g" % (E, len(rec), worst))
    assert worst < TOL, worst


def test_hidden_out_takes_the_last_pass_and_an_armed_gate_record_is_refused():
    """ic3_env_set_hidden_out: h', c' of the LAST pass go to the armed rows and the rows handed in keep their bits;
    ic3_env_set_record_out: the npasses launch keeps no gate record — refused with the message the call has at 64 / 128."""
    w = dict(CASES['pp_p2'], E=3)
    E, N = w['E'], w['N']
    res = []
    for armed in (False, True):
        env = _env(w, 5, 11)
        pol = HostPolicy(env, _params(w, env.obs_dim, 6), H, w['heads'], gate_split=True, passes=2)
        rng = np.random.default_rng(3)
        h = (rng.standard_normal((E * N, H)) * 0.3).astype(np.float32)
        c = (rng.standard_normal((E * N, H)) * 0.3).astype(np.float32)
        h0, c0 = h.copy(), c.copy()
        gate = np.ones((E, N), np.int32)
        h2 = np.full_like(h, np.nan)
        c2 = np.full_like(c, np.nan)
        if armed:
            check(env.lib.ic3_env_set_hidden_out(env._h, p(h2), p(c2)))
        out = pol.step(env, h, c, None, gate, with_obs=False)[0]
        if armed:
            np.testing.assert_array_equal(h, h0)
            np.testing.assert_array_equal(c, c0)
            res.append((out, h2, c2))
            # the gate record: refused before any launch, the one-shot consumed
            g = np.full((E * N, 4 * H), np.nan, np.float32)
            check(env.lib.ic3_env_set_record_out(env._h, p(g), None))
            before = env.raw_state()
            out2 = np.full_like(out, np.nan)
            act = np.full((2, E, N), -7, np.int32)
            rew, done = np.full((E, N), np.nan, np.float32), np.full((E,), -7, np.int32)
            rc = env.lib.ic3_policy_step(env._h, C.byref(pol.struct), p(h), p(c), None, p(gate), p(out2), p(act), None, p(rew), p(done),
                                         None, None, None)
            msg = env.lib.ic3_last_error().decode()
            assert rc == -38 and msg.startswith("ic3_env_set_record_out: the gate record needs gate_split, one communication pass"), (rc, msg)
            assert np.isnan(g).all() and np.isnan(out2).all() and (act == -7).all() and np.isnan(rew).all() and (done == -7).all()
            np.testing.assert_array_equal(env.raw_state(), before)
            np.testing.assert_array_equal(h, h0)
        else:
            res.append((out, h.copy(), c.copy()))
        env.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    assert np.isfinite(res[1][1]).all() and np.isfinite(res[1][2]).all()
