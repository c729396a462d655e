"""CPU: ic3_bptt_backward on an ic3_bptt_walk descriptor — a comm_zero window of the LSTM backward through time with its T steps walked
in ONE launch (lstm_gates_bwd_walk_kernel, csrc/gates_bwd.hip) — on the host build of the product's own sources
(tests/host/libic3rollout_host.so), against the same call on the untagged ic3_bptt (comm_zero = 1, the ring, one chain: a gate launch
and the copy of d h_prev per step) BIT FOR BIT on identical inputs from bptt_window_ref.make_window: the gate record (dgates), the
d inp columns of every ring slot (the d h_prev columns keep their NaN pre-fill: the walk does not write them), dh and dc leaving the
window, every row of the bias partials (pre-filled with random values: they are added to) and the encoder's dWt / db through the
window finish.  R = 390 (PP, 3 agents, E = 130: a ragged last tile) and 650 (TJ-easy, 5 agents); T = 1 all detached, detach points at
the last step's successor and inside, none with dh / dc arriving; collection cuts over two windows on one set of partials; OT 1 and
16; hid 64 / 128 / 256 (256 on the 32-agent dim-6 PP grid), and each width with max_workgroups = 2, where a workgroup walks several
tiles.  The case of test_host_bptt_window_cpu's 'C-comm-zero' shape is also held to the float64 window backward at that case's bars.
And what the descriptor refuses, with every output left as it was."""
import ctypes as C

import numpy as np
import pytest

import bptt_window_ref as ref
from bptt_window_bars import BARS
from host_abi_util import HostEnv, check, host_lib, p

CASES = {
    # the shape, seed and steps of test_host_bptt_window_cpu.CASES['C-comm-zero']: also against float64
    'C-comm-zero': dict(kind='pp', E=130, H=64, T=3, gap=2, f64='host/C-comm-zero'),
    'h64-tj-T1-gap1-OT1': dict(kind='tj', E=130, H=64, T=1, gap=1, OT=1),
    'h64-pp-T5-gap2-OT16': dict(kind='pp', E=130, H=64, T=5, gap=2, OT=16),
    'h64-tj-collect-two-windows': dict(kind='tj', E=130, H=64, T=4, collect=True, windows=((2, 2), (0, 2))),
    'h64-pp-T3-gap3-two-workgroups': dict(kind='pp', E=130, H=64, T=3, gap=3, wgs=2),
    'h128-pp-T2-gap0-arriving': dict(kind='pp', E=130, H=128, T=2, gap=0),
    'h128-pp-T2-collect-two-workgroups': dict(kind='pp', E=130, H=128, T=2, collect=True, wgs=2),
    'h256-pp-n32-T2-gap2': dict(kind='pp32', E=3, H=256, T=2, gap=2),
    'h256-pp-n32-T2-collect-two-workgroups': dict(kind='pp32', E=5, H=256, T=2, collect=True, wgs=2),
}


def _env(kind, E):
    if kind == 'pp':
        return HostEnv.pp(3, 6, 1, 'mixed', E, seed=3)
    if kind == 'pp32':                                           # (32 agents need 33 cells: dim 6 is the smallest grid)
        return HostEnv.pp(32, 6, 1, 'mixed', E, seed=3)
    return HostEnv.tj(5, 6, 1, 'easy', E, seed=3, add_rate_min=0.6, add_rate_max=0.6)


def _states(env, T):
    from test_host_abi_cpu import _play
    snaps, obs = [], []
    for t in range(T):
        _play(env, 2 + t, 70 + t)
        snaps.append(env.snapshot())
        obs.append(env.observe().reshape(env.E * env.N, env.obs_dim).astype(np.float64))
    return np.ascontiguousarray(np.stack(snaps)), obs


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _fill(b, binding, walk, lib, env, w, t0, n, snaps, bufs, gap, enc_first, wgs=0):
    """The fields of one call on steps [t0, t0 + n) of the window: an untagged ic3_bptt with comm_zero / the ring / one chain, or the
    walk's descriptor."""
    E, N, H, OT = w['E'], w['N'], w['H'], w['OT']
    R = E * N
    assert b.struct_size == C.sizeof(b)
    b.T, b.E, b.N, b.H, b.OT, b.detach_gap, b.enc_first = n, E, N, H, OT, gap, enc_first
    if walk:
        assert b.magic == binding.BpttWalk.MAGIC
        b.max_workgroups = wgs
    else:
        b.mode_avg, b.comm_zero, b.two_chains = 1, 1, 0
    sn = snaps[t0:t0 + n]
    b.gates, b.dxh = bufs['gates'][t0:].ctypes.data, bufs['dxh'][t0:].ctypes.data
    b.hs, b.cs, b.dhead = w['hs'][t0:].ctypes.data, w['cs'][t0:].ctypes.data, w['dhead'][t0:].ctypes.data
    b.snaps, b.snap_words = sn.ctypes.data, snaps.shape[1]
    if w['row_live'] is not None:
        b.row_live, b.row_keep = w['row_live'][t0:].ctypes.data, w['row_keep'][t0:].ctypes.data
    b.lstm_wp3_bwd, b.w_heads = bufs['wb3'].ctypes.data, w['w_heads'].ctypes.data
    b.dh, b.dc, b.dbias_partials = bufs['dh'].ctypes.data, bufs['dc'].ctypes.data, bufs['bias'].ctypes.data
    b.enc_work, b.dxh_step = bufs['work'].ctypes.data, R * 2 * H
    return b, sn


def _buffers(lib, env, w, T):
    R, H = w['E'] * w['N'], w['H']
    wb3 = np.zeros(3 * 4 * H * 2 * H, np.uint16)
    check(lib.ic3_policy_pack_split_bwd(p(w['w_ih']), p(w['w_hh']), p(wb3), H, None))
    n = int(lib.ic3_env_encode_backward_window_work(env._h, H))
    assert n > 0
    return dict(gates=w['gates'].copy(), dh=w['dh'].copy(), dc=w['dc'].copy(), dxh=np.full((T, R, 2 * H), np.nan, np.float32),
                bias=np.random.default_rng(99).standard_normal(((R + 63) // 64, 4 * H)).astype(np.float32), wb3=wb3,
                work=np.full((n,), np.nan, np.float32))


def _run(lib, binding, env, cfg, w, snaps, walk):
    """The case's window(s), the later one first, on fresh buffers; what the call(s) and the encoder's finish left."""
    T, H = cfg['T'], cfg['H']
    bufs = _buffers(lib, env, w, T)
    for k, (t0, n) in enumerate(cfg.get('windows', ((0, T),))):
        if k and w['row_keep'] is not None:                      # (the caller's part: what crosses the border between two windows)
            bufs['dh'] *= w['row_keep'][t0 + n - 1][:, None]
            bufs['dc'] *= w['row_keep'][t0 + n - 1][:, None]
        b, keep = _fill((binding.BpttWalk if walk else binding.Bptt)(), binding, walk, lib, env, w, t0, n, snaps, bufs, cfg.get('gap', 0),
                        int(k == 0), cfg.get('wgs', 0))
        check(lib.ic3_bptt_backward(env._h, C.byref(b), None))
    dwt = np.full((env.obs_dim, H), np.nan, np.float32)
    db = np.full((H,), np.nan, np.float32)
    check(lib.ic3_env_encode_backward_window_finish(env._h, H, p(dwt), p(db), p(bufs['work']), None))
    return dict(dgates=bufs['gates'], dh=bufs['dh'], dc=bufs['dc'], dinp=np.ascontiguousarray(bufs['dxh'][..., :H]),
                bias=bufs['bias'], enc_dwt=dwt, enc_db=db), bufs['dxh'][..., H:]


@pytest.mark.parametrize("name", list(CASES))
def test_walk_is_the_per_step_call_bit_for_bit(name):
    from ic3net_amd import _lib as binding
    lib = host_lib()
    cfg = CASES[name]
    env = _env(cfg['kind'], cfg['E'])
    T, H, OT = cfg['T'], cfg['H'], cfg.get('OT', 6)
    w = ref.make_window(sum(map(ord, name)), T, env.E, env.N, H, OT, collect=cfg.get('collect', False))
    snaps, obs = _states(env, T)
    tiles = (env.E * env.N + 63) // 64
    assert tiles > cfg.get('wgs', tiles - 1) >= 1                # (more than one tile; capped: more tiles than workgroups)
    steps, steps_dhp = _run(lib, binding, env, cfg, w, snaps, walk=False)
    walk, walk_dhp = _run(lib, binding, env, cfg, w, snaps, walk=True)
    assert not np.isnan(steps_dhp).any() and np.isnan(walk_dhp).all()    # the d h_prev half of the ring: written / left alone
    assert not np.isnan(walk['dinp']).any() and not np.array_equal(walk['dgates'], w['gates'])
    bad = [k for k in steps if not _same_bits(steps[k], walk[k])]
    assert not bad, "%s: the walk differs from the per-step call in %r" % (name, bad)
    if cfg.get('f64'):                                           # ... and against the float64 window backward, at the existing bars
        want = ref.reference_of(w, obs=obs, detach_gap=cfg.get('gap', 0), comm_zero=True)
        bias0 = np.random.default_rng(99).standard_normal((tiles, 4 * H)).astype(np.float32)
        errs = dict(dgates=ref.rel_err(walk['dgates'], want['dgates']), dh=ref.rel_err(walk['dh'], want['dh']),
                    dc=ref.rel_err(walk['dc'], want['dc']), dxh=ref.rel_err(walk['dinp'], want['dxh'][..., :H]),
                    dbias_rows=ref.rel_err(walk['bias'], bias0.astype(np.float64) + want['dbias_rows']),
                    enc_dwt=ref.rel_err(walk['enc_dwt'], want['enc_dwt']), enc_db=ref.rel_err(walk['enc_db'], want['enc_db']))
        Q = T * env.E * env.N
        dW0 = np.random.default_rng(5).standard_normal((2 * H, 4 * H)).astype(np.float32)
        dW = dW0.copy()
        scratch = np.zeros(lib.ic3_lstm_weight_grad_scratch_floats(Q, H), np.float32)
        check(lib.ic3_lstm_weight_grad(p(w['inp']), H, p(w['hs']), p(walk['dgates']), p(w['row_live']), Q, H, p(dW), 1, 1, p(scratch), None))
        errs['dW'] = ref.rel_err(dW, dW0.astype(np.float64) + want['dW'])
        bars = BARS[cfg['f64']]
        for k in sorted(errs):
            print("lstm-walk %s %s %.3e (bar %.3e)" % (cfg['f64'], k, errs[k], bars[k]))
        over = {k: (v, bars[k]) for k, v in errs.items() if not v <= bars[k]}
        assert not over, "%s: (measured, bar) %r" % (name, over)
    env.close()


REFUSALS = {
    # what, errno, a piece of the message
    'another-size': (-22, b"ic3_bptt_walk has"),
    'null-dc': (-22, b"null argument"),
    'null-w-heads': (-22, b"null argument"),
    'dxh-step-short': (-22, b"dxh_step"),
    'gap-with-row-keep': (-22, b"row_keep"),
    'OT-0': (-22, b"OT"),
    'OT-17': (-22, b"OT"),
    'H-32': (-38, b"64 / 128 / 256"),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_walk_refusals_leave_everything_untouched(what):
    """Each refusal of the descriptor: its errno, a message that begins with the descriptor's name, and the record, dh / dc, the bias
    partials, the ring and the encoder's sums as they were.  (A configuration without the encoder's window form shares its check and
    message with the short ring step: at the sizes the call takes, every grid with the partial-sums form has the window form.)  A tagged descriptor of another size is refused whatever else it holds,
    and runs once its size is corrected."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    want, msg = REFUSALS[what]
    env = _env('pp', 30)
    H = 32 if what == 'H-32' else 64
    OT = dict({'OT-0': 0, 'OT-17': 17}).get(what, 6)
    T = 2
    w = ref.make_window(3, T, env.E, env.N, H, max(OT, 1), collect=(what == 'gap-with-row-keep'))
    w['OT'] = OT
    snaps, _ = _states(env, T)
    R = env.E * env.N
    if what == 'H-32':                                           # (no packed planes and no encoder sums at a size the library lacks)
        wb3 = np.zeros(3 * 4 * H * 2 * H, np.uint16)
        bufs = dict(gates=w['gates'].copy(), dh=w['dh'].copy(), dc=w['dc'].copy(), dxh=np.full((T, R, 2 * H), np.nan, np.float32),
                    bias=np.ones(((R + 63) // 64, 4 * H), np.float32), wb3=wb3, work=np.full((64,), np.nan, np.float32))
    else:
        bufs = _buffers(lib, env, w, T)
    bias0 = bufs['bias'].copy()
    b, keep = _fill(binding.BpttWalk(), binding, True, lib, env, w, 0, T, snaps, bufs, 2 if what == 'gap-with-row-keep' else 0, 1)
    if what == 'another-size':
        b.struct_size = C.sizeof(binding.Bptt)                   # (the untagged struct's size under the tag)
    elif what == 'null-dc':
        b.dc = None
    elif what == 'null-w-heads':
        b.w_heads = None
    elif what == 'dxh-step-short':
        b.dxh_step = R * 2 * H - 4
    assert lib.ic3_bptt_backward(env._h, C.byref(b), None) == want
    err = lib.ic3_last_error()
    assert err.startswith(b"ic3_bptt_backward (ic3_bptt_walk)") and msg in err, err
    assert _same_bits(bufs['gates'], w['gates']) and _same_bits(bufs['dh'], w['dh']) and _same_bits(bufs['dc'], w['dc'])
    assert _same_bits(bufs['bias'], bias0) and np.isnan(bufs['dxh']).all() and np.isnan(bufs['work']).all()
    if what == 'another-size':                                   # ... and the same descriptor at its own size runs
        b.struct_size = C.sizeof(b)
        check(lib.ic3_bptt_backward(env._h, C.byref(b), None))
        assert not np.isnan(bufs['dxh'][..., :H]).any() and not _same_bits(bufs['gates'], w['gates'])
    env.close()
