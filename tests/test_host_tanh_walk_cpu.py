"""CPU: ic3_rnn_backward_wide on an ic3_rnn_bptt_walk descriptor — the tanh recurrence's window backward with its T steps walked in
ONE launch (rnn_tanh_bwd_walk_kernel) — on the host build of the product's own sources (tests/host/libic3rollout_host.so), against
the same call on the untagged ic3_rnn_bptt (one launch per step) BIT FOR BIT: the dz ring, dh leaving the window, every partial row
(zeroed partials; one tile per workgroup at these sizes), a2_grad and the encoder's dWt / db through the matching finish.  The cases
are test_host_tanh_window_cpu.RNN_CASES (R = 150 / 90: ragged last tiles; T = 1 all detach; a detach at the window's last step and
inside it; h_last separate; OT 1 and 16; collection cuts; two windows on one set of accumulators) plus a lock-step and a collection
window at hid 256 (the shapes of test_host_tanh_window_h256_cpu).  The walk is also held to the float64 window backward of
tests/tanh_window_ref.py at the per-step path's own bars, looked up under the existing case names.  And what the entries refuse,
with every output buffer left untouched."""
import ctypes as C

import numpy as np
import pytest

import tanh_window_ref as ref
from host_abi_util import check, host_lib
from tanh_window_bars import BARS as BARS_64_128
from tanh_window_h256_bars import BARS as BARS_256
from test_host_tanh_window_cpu import RNN_CASES, _enc_finish, _enc_work, _env, _record_states
from test_host_tanh_window_h256_cpu import RNN_CASES as RNN_CASES_256

CASES = dict(RNN_CASES)
for _name in ('rnn-A-h256-T3-gap2', 'rnn-B-h256-collect-two-windows'):      # one lock-step, one collection case at hid 256
    CASES[_name] = dict(RNN_CASES_256[_name], H=256)
BARS = dict(BARS_64_128, **BARS_256)


def _descriptor(binding, walk):
    b = (binding.RnnBpttWalk if walk else binding.RnnBptt)()
    assert b.struct_size == C.sizeof(b) and C.sizeof(binding.RnnBpttWalk) != C.sizeof(binding.RnnBptt) == 160
    if walk:
        assert b.magic == binding.RnnBpttWalk.MAGIC == 0x4b4c4157 and binding.RnnBpttWalk.magic.offset == binding.RnnBptt.T.offset
    return b


def _run(lib, binding, env, cfg, w, snaps, walk):
    """The case's window(s) through ic3_rnn_backward_wide on the untagged descriptor (walk = False) or the walk's, on zeroed
    partials and a zeroed a2_grad, and the encoder's finish: dict of what the call left."""
    T, H, OT, gap = cfg['T'], cfg['H'], cfg.get('OT', 6), cfg.get('gap', 0)
    E, N = env.E, env.N
    R = E * N
    enc_window = cfg.get('enc_window', True)
    nparts = (R + 63) // 64
    assert lib.ic3_rnn_backward_wide_partials(R, H) == nparts    # (one tile per workgroup: the rows of both paths correspond)
    parts, a2g, dh = np.zeros((nparts, H), np.float32), np.zeros((H, H), np.float32), w['dh'].copy()
    dz = np.full((T, R, H), np.nan, np.float32)
    work = _enc_work(lib, env, H, enc_window)
    for k, (t0, n) in enumerate(cfg.get('windows', ((0, T),))):
        b = _descriptor(binding, walk)
        b.T, b.E, b.N, b.H, b.OT = n, E, N, H, OT
        b.detach_gap, b.enc_first, b.enc_window = gap, int(k == 0), int(enc_window)
        hs, dhead, sn, ring = w['hs'][t0:], w['dhead'][t0:t0 + n], snaps[t0:t0 + n], dz[t0:t0 + n]
        b.hs, b.dhead, b.snaps, b.snap_words = hs.ctypes.data, dhead.ctypes.data, sn.ctypes.data, snaps.shape[1]
        b.h_last = w['h_last'].ctypes.data if (w['h_last'] is not None and t0 + n == T) else None
        b.a2, b.w_heads = w['a2'].ctypes.data, w['w_heads'].ctypes.data
        if w['row_live'] is not None:
            live, keep = w['row_live'][t0:t0 + n], w['row_keep'][t0:t0 + n]
            b.row_live, b.row_keep = live.ctypes.data, keep.ctypes.data
            if k:                                                # (the caller's part: what crosses the border between two windows)
                dh *= w['row_keep'][t0 + n - 1][:, None]
        b.dh, b.dz, b.dbias_partials, b.enc_work = dh.ctypes.data, ring.ctypes.data, parts.ctypes.data, work.ctypes.data
        if cfg.get('a2', True):
            scratch = np.full(lib.ic3_rnn_weight_grad_wide_scratch_floats(n * R, H), np.nan, np.float32)
            b.a2_grad, b.wgrad_scratch = a2g.ctypes.data, scratch.ctypes.data
        check(lib.ic3_rnn_backward_wide(env._h, C.byref(b), None))
    dwt, db = _enc_finish(lib, env, H, work, enc_window)
    return dict(dz=dz, dh=dh, parts=parts, a2_grad=a2g, enc_dwt=dwt, enc_db=db)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", list(CASES))
def test_walk_is_the_per_step_call_bit_for_bit(name):
    from ic3net_amd import _lib as binding
    lib = host_lib()
    cfg = CASES[name]
    env = _env(cfg['kind'], cfg['E'])
    T, H, OT, gap = cfg['T'], cfg['H'], cfg.get('OT', 6), cfg.get('gap', 0)
    w = ref.make_rnn_window(sum(map(ord, name)), T, env.E, env.N, H, OT, collect=cfg.get('collect', False),
                            h_last=cfg.get('h_last', 'slot'))
    snaps, obs = _record_states(env, T)
    steps = _run(lib, binding, env, cfg, w, snaps, walk=False)
    walk = _run(lib, binding, env, cfg, w, snaps, walk=True)
    assert not np.isnan(walk['dz']).any()
    bad = [k for k in steps if not _same_bits(steps[k], walk[k])]
    assert not bad, "%s: the walk differs from the per-step call in %r" % (name, bad)
    if not cfg.get('a2', True):
        assert not walk['a2_grad'].any()
    # the walk against the float64 window backward, at the per-step path's bars for this case
    want = ref.rnn_reference_of(w, obs=obs, detach_gap=gap)
    zeros = np.zeros_like(walk['parts'])
    errs = ref.rnn_errors(want, walk['dz'], walk['dh'], walk['parts'], zeros, walk['a2_grad'] if cfg.get('a2', True) else None,
                          np.zeros_like(walk['a2_grad']))
    assert 'dbias_tiles' in errs
    errs['enc_dwt'], errs['enc_db'] = ref.rel_err(walk['enc_dwt'], want['enc_dwt']), ref.rel_err(walk['enc_db'], want['enc_db'])
    env.close()
    bars = BARS['host/' + name]
    for k in sorted(errs):
        print("tanh-walk host/%s %s %.3e (bar %.3e)" % (name, k, errs[k], bars[k]))
    over = {k: (v, bars[k]) for k, v in errs.items() if not v <= bars[k]}
    assert not over, "%s: (measured, bar) %r" % (name, over)


def _refusal_buffers(R, H, T, OT):
    rng = np.random.default_rng(7)
    ins = dict(hs=np.tanh(rng.standard_normal((T + 1, R, H))).astype(np.float32), dhead=rng.standard_normal((T, R, OT)).astype(np.float32),
               a2=rng.standard_normal((H, H)).astype(np.float32), w_heads=rng.standard_normal((OT, H)).astype(np.float32))
    outs = dict(dh=np.full((R, H), np.nan, np.float32), dz=np.full((T, R, H), np.nan, np.float32),
                parts=np.full(((R + 63) // 64, H), np.nan, np.float32), a2_grad=np.full((H, H), np.nan, np.float32),
                scratch=np.full((4 * H * H,), np.nan, np.float32))
    return ins, outs


@pytest.mark.parametrize("what", ['another-size', 'narrow-entry', 'H-32', 'OT-17'])
def test_walk_refusals_leave_the_outputs_untouched(what):
    """A tagged descriptor of another size: -EINVAL (the size is what is checked, whatever else it holds); the narrow entry does not
    know the tag and answers -EINVAL on the size, as it does today for any descriptor of 168 bytes; hid 32: -ENOSYS; 17 output
    columns: -EINVAL.  dh, dz, the partials, a2_grad, the weight gradient's scratch and the encoder's sums keep their NaN pre-fill."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    env = _env('pp', 9)
    R, T = env.E * env.N, 2
    H, OT = (32 if what == 'H-32' else 64), (17 if what == 'OT-17' else 6)
    ins, outs = _refusal_buffers(R, H, T, OT)
    snaps, _ = _record_states(env, T)
    work = _enc_work(lib, env, 64, True)
    b = binding.RnnBpttWalk()
    b.T, b.E, b.N, b.H, b.OT, b.enc_first, b.enc_window = T, env.E, env.N, H, OT, 1, 1
    b.hs, b.dhead, b.a2, b.w_heads = (ins[k].ctypes.data for k in ('hs', 'dhead', 'a2', 'w_heads'))
    b.snaps, b.snap_words = snaps.ctypes.data, snaps.shape[1]
    b.dh, b.dz, b.dbias_partials, b.a2_grad, b.wgrad_scratch = (outs[k].ctypes.data for k in ('dh', 'dz', 'parts', 'a2_grad', 'scratch'))
    b.enc_work = work.ctypes.data
    entry, want, msg = lib.ic3_rnn_backward_wide, -22, b"ic3_rnn_bptt_walk has"
    if what == 'another-size':
        b.struct_size = C.sizeof(binding.RnnBptt)                # (the untagged struct's size under the tag)
    elif what == 'narrow-entry':
        entry, msg = lib.ic3_rnn_backward, b"ic3_rnn_bptt has 168 bytes"
    elif what == 'H-32':
        want, msg = -38, b"64 / 128 / 256"
    else:
        msg = b"OT"
    assert entry(env._h, C.byref(b), None) == want
    assert msg in lib.ic3_last_error(), lib.ic3_last_error()
    for k, v in outs.items():
        assert np.isnan(v).all(), k
    assert np.isnan(work).all()
    if what == 'another-size':                                   # ... and the same descriptor at its own size runs
        b.struct_size = C.sizeof(b)
        outs['dh'][:], outs['parts'][:], outs['a2_grad'][:] = 0, 0, 0
        check(entry(env._h, C.byref(b), None))
        assert not np.isnan(outs['dz']).any() and not np.isnan(outs['dh']).any()
    env.close()
