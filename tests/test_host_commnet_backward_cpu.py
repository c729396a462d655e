"""CPU: the non-recurrent CommNet module's window backward (ic3_commnet_backward, csrc/bptt_kernels.hip + the recording forward of
csrc/commnet_fwd.hip) on the host build of the product's own sources (tests/host/libic3rollout_host.so: the matrix-core kernels
run on the stand-in runtime) — the pass launch and the recording forward alone, the whole entry on a Predator-Prey and a
Traffic-Junction env, the struct_size handshake and refusal codes of ic3_commnet_bptt, and a window run in chunks against the
same window in one.  Reference: tests/commnet_window_ref.py (float64); bars: tests/commnet_window_bars.py."""
import ctypes as C

import numpy as np
import pytest

import commnet_window_ref as ref
from host_abi_util import HostEnv, check, host_lib, p

_f32 = ref._f32


def _pack(lib, w):
    """ic3_commnet_pack of every pass: wp (P, 2 H H)"""
    H, P = w['H'], w['P']
    wp = np.full((P, 2 * H * H), np.nan, np.float32)
    for i in range(P):
        check(lib.ic3_commnet_pack(p(w['c_w'][i]), p(w['f_w'][i]), p(wp[i]), H, None))
    return wp


# ---- the pass launch alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Q,OT,with_dh,with_heads", [(64, 70, 6, False, True), (64, 130, 6, True, False), (128, 129, 16, True, True)])
def test_pass_backward_against_float64(H, Q, OT, with_dh, with_heads):
    """ic3_commnet_pass_backward, Q not a multiple of the 64-row tile, with and without dh_in / dhead: dz (both copies), dz . F, dx
    written and then added to, the partials' column sums — against float64."""
    lib = host_lib()
    rng = np.random.default_rng(H * 1000 + Q)
    rn = lambda *s: rng.standard_normal(s)
    h = _f32(np.tanh(rn(Q, H)))
    dh_in = _f32(rn(Q, H)) if with_dh else None
    dhead, w_heads = (_f32(rn(Q, OT)), _f32(rn(OT, H) / H ** 0.5)) if with_heads else (None, None)
    fw = _f32(rn(H, H) / H ** 0.5)
    v = (dh_in.astype(np.float64) if with_dh else 0.0) + (dhead.astype(np.float64) @ w_heads.astype(np.float64) if with_heads else 0.0)
    want_dz = v * (1.0 - h.astype(np.float64) ** 2)
    want_zf = want_dz @ fw.astype(np.float64)
    nparts = lib.ic3_commnet_pass_backward_partials(Q, H)
    assert 1 <= nparts <= (Q + 63) // 64
    dxh, dz, dx = (np.full(s, np.nan, np.float32) for s in ((Q, 2 * H), (Q, H), (Q, H)))
    parts = np.full((nparts, H), np.nan, np.float32)
    call = lambda add, acc: check(lib.ic3_commnet_pass_backward(p(dh_in), p(h), p(dhead), p(w_heads), OT, p(fw), p(dxh), p(dz), p(dx), add,
                                                                p(parts), acc, Q, H, None))
    assert call(0, 0) == nparts
    case = "host_pass_H%d_Q%d_%s%s" % (H, Q, 'd' if with_dh else '', 'h' if with_heads else '')
    assert np.array_equal(dxh[:, :H], dz)                      # the two copies of dz
    errs = dict(dz=ref.rel_err(dz, want_dz), dzF=ref.rel_err(dxh[:, H:], want_zf), dx=ref.rel_err(dx, want_dz),
                bias_cols=ref.rel_err(parts.astype(np.float64).sum(0), want_dz.sum(0)))
    # accumulating: dx += dz on top of what it holds, the partials added to
    dx0 = _f32(rn(Q, H))
    dx[:] = dx0
    assert call(1, 1) == nparts
    errs['dx_add'] = ref.rel_err(dx, dx0.astype(np.float64) + want_dz)
    errs['bias_cols_acc'] = ref.rel_err(parts.astype(np.float64).sum(0), 2 * want_dz.sum(0))
    ref.check(case, errs)


def test_pass_backward_refusals():
    """-ENOSYS for another hid_size or more than 16 output columns, -EINVAL for a null buffer or OT < 1 with dhead; the partials
    query answers 0 where the launch refuses."""
    lib = host_lib()
    Q = 8
    buf = lambda *s: np.zeros(s, np.float32)
    for H, OT, want in ((32, 6, -38), (96, 6, -38), (128, 17, -38), (128, 0, -22)):
        h, d, w, fw = buf(Q, H), buf(Q, max(OT, 1)), buf(max(OT, 1), H), buf(H, H)
        dxh, dz, dx, parts = buf(Q, 2 * H), buf(Q, H), buf(Q, H), buf(1, H)
        assert lib.ic3_commnet_pass_backward(None, p(h), p(d), p(w), OT, p(fw), p(dxh), p(dz), p(dx), 0, p(parts), 0, Q, H, None) == want
    h = buf(Q, 64)
    assert lib.ic3_commnet_pass_backward(None, p(h), None, None, 0, None, None, None, None, 0, None, 0, Q, 64, None) == -22
    assert lib.ic3_commnet_pass_backward_partials(100, 96) == 0
    assert lib.ic3_commnet_pass_backward_partials(0, 128) == 0
    assert lib.ic3_commnet_pass_backward_partials(100, 256) >= 1


# ---- the recording forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,P,E,N,mode_avg,comm_zero", [(64, 2, 9, 5, True, False), (64, 3, 7, 3, False, False), (128, 2, 5, 10, True, True)])
def test_forward_record_against_forward_and_float64(H, P, E, N, mode_avg, comm_zero):
    """ic3_commnet_forward_record: slot P of the ring and its h_out / out are ic3_commnet_forward's, bit for bit; slot 0 = tanh(enc)
    and the passes between against float64; slot 0 written over enc; out NULL runs without the heads' arguments."""
    lib = host_lib()
    rng = np.random.default_rng(H + P + E)
    R, OT = E * N, 6
    w = ref.make_weights(11 + P, H, P, OT, 7)
    wp = _pack(lib, w)
    enc = _f32(rng.standard_normal((R, H)))
    alive, gate = ref.make_masks(rng, 1, E, N, dead=0.2, gated=0.3)
    head_b = _f32(rng.standard_normal(OT) * 0.1)
    sizes = (C.c_int32 * 1)(OT - 1)
    out0, h0 = np.full((R, OT), np.nan, np.float32), np.full((R, H), np.nan, np.float32)
    check(lib.ic3_commnet_forward(p(enc), E, N, H, P, p(wp), None, p(w['bias']), p(w['w_heads']), p(head_b), sizes, 1, int(mode_avg),
                                  int(comm_zero), p(alive), p(gate), p(out0), p(h0), None))
    out1, h1 = np.full((R, OT), np.nan, np.float32), np.full((R, H), np.nan, np.float32)
    ring = np.full((P + 1, R, H), np.nan, np.float32)
    check(lib.ic3_commnet_forward_record(p(enc), E, N, H, P, p(wp), None, p(w['bias']), p(w['w_heads']), p(head_b), sizes, 1,
                                         int(mode_avg), int(comm_zero), p(alive), p(gate), p(out1), p(h1), p(ring), None))
    assert np.array_equal(out0, out1) and np.array_equal(h0, h1) and np.array_equal(ring[P], h0)
    want = ref.window_backward([enc], None, None, w['f_w'], w['c_w'], w['bias'], w['w_heads'], np.zeros((1, R, OT)), E, N, alive=alive,
                               gate=gate, mode_avg=mode_avg, comm_zero=comm_zero)['h_pass'][:, 0]
    ref.check("host_record_H%d_P%d" % (H, P), dict(h_pass=ref.rel_err(ring, want)))
    # in place over enc, no heads
    ring2 = np.full((P + 1, R, H), np.nan, np.float32)
    ring2[0] = enc
    check(lib.ic3_commnet_forward_record(p(ring2), E, N, H, P, p(wp), None, p(w['bias']), None, None, None, 0, int(mode_avg),
                                         int(comm_zero), p(alive), p(gate), None, None, p(ring2), None))
    assert np.array_equal(ring2, ring)
    assert lib.ic3_commnet_forward_record(p(enc), E, N, H, P, p(wp), None, p(w['bias']), None, None, None, 0, 1, 0, None, None, None,
                                          None, None, None) == -22
    assert lib.ic3_commnet_forward_record(p(enc), E, N, 96, P, p(wp), None, p(w['bias']), None, None, None, 0, 1, 0, None, None, None,
                                          None, p(ring2), None) == -38


# ---- the whole entry ----------------------------------------------------------------------------------------------------------
class _Window(object):
    """A window of T played states of `env`, random masks and dhead, the buffers of one ic3_commnet_backward call"""

    def __init__(self, env, w, T, seed, mode_avg=True, comm_zero=False, gates=True, dead=0.2):
        from test_host_abi_cpu import _play
        self.env, self.w, self.T, self.mode_avg, self.comm_zero = env, w, T, mode_avg, comm_zero
        rng = np.random.default_rng(seed)
        self.E, self.N, self.R = env.E, env.N, env.E * env.N
        snaps, self.obs = [], []
        for t in range(T):
            _play(env, 2 + t, seed + t)
            snaps.append(env.snapshot())
            self.obs.append(env.observe().reshape(self.R, env.obs_dim).astype(np.float64))
        self.snaps = np.ascontiguousarray(np.stack(snaps))
        self.alive, gate = ref.make_masks(rng, T, self.E, self.N, dead=dead, gated=0.3)
        self.gate = gate if gates else None
        self.dhead = _f32(rng.standard_normal((T, self.R, w['OT'])))
        self.wp = _pack(host_lib(), w)

    def reference(self):
        return ref.reference_of(self.w, self.obs, self.dhead, self.E, self.N, alive=self.alive, gate=self.gate, mode_avg=self.mode_avg,
                                comm_zero=self.comm_zero)

    def run(self, max_chunk_steps=0, enc_window=1, seed=0):
        """-> dict of what the call left: per-pass gradients (on top of a random pre-fill, returned too), the rings, the encoder's"""
        from ic3net_amd import _lib as binding
        lib, env, w, T = host_lib(), self.env, self.w, self.T
        H, P, OT, R = w['H'], w['P'], w['OT'], self.R
        rng = np.random.default_rng(1000 + seed)
        tc = lib.ic3_commnet_backward_chunk_steps(env._h, T, H, max_chunk_steps)
        assert 1 <= tc <= T and (max_chunk_steps == 0 or tc <= max_chunk_steps)
        Qc = tc * R
        nan = lambda *s: np.full(s, np.nan, np.float32)
        o = dict(tc=tc, h_pass=nan(P + 1, Qc, H), dxh=nan(Qc, 2 * H), dz=nan(Qc, H), dx=nan(Qc, H), de=nan(Qc, H), dh=nan(Qc, H))
        nscr = lib.ic3_commnet_backward_scratch_floats(env._h, T, H, max_chunk_steps)
        assert nscr > 0
        scratch = nan(nscr)
        nw = int(lib.ic3_env_encode_backward_window_work(env._h, H) if enc_window else lib.ic3_env_encode_backward_work(env._h, H))
        assert nw > 0
        work = nan(nw)
        pre = lambda *s: _f32(rng.standard_normal(s))
        o['f_grad'], o['c_grad'], o['bias_grad'] = [pre(H, H) for _ in range(P)], [pre(H, H) for _ in range(P)], [pre(H) for _ in range(P)]
        o['heads_w'], o['heads_b'] = pre(OT, H), pre(OT)
        o['pre'] = {k: [a.astype(np.float64) for a in o[k]] if isinstance(o[k], list) else o[k].astype(np.float64)
                    for k in ('f_grad', 'c_grad', 'bias_grad', 'heads_w', 'heads_b')}
        arr = lambda lst: (C.c_void_p * P)(*[a.ctypes.data for a in lst])
        keep = [arr(w['f_w']), arr(w['c_w']), arr(o['f_grad']), arr(o['c_grad']), arr(o['bias_grad'])]
        b = binding.CommnetBptt()
        b.struct_size = C.sizeof(b)
        b.T, b.E, b.N, b.H, b.OT, b.passes = T, self.E, self.N, H, OT, P
        b.mode_avg, b.comm_zero, b.enc_first, b.enc_window, b.max_chunk_steps = int(self.mode_avg), int(self.comm_zero), 1, enc_window, max_chunk_steps
        b.dhead, b.snaps, b.snap_words = self.dhead.ctypes.data, self.snaps.ctypes.data, self.snaps.shape[1]
        b.alive = self.alive.ctypes.data
        b.gate = self.gate.ctypes.data if self.gate is not None else None
        b.enc_wt, b.enc_bias, b.loc_table = w['enc_wt'].ctypes.data, w['enc_bias'].ctypes.data, None
        b.wp, b.wp3, b.bias, b.w_heads = self.wp.ctypes.data, None, w['bias'].ctypes.data, w['w_heads'].ctypes.data
        b.f_weight, b.c_weight, b.f_grad, b.c_grad, b.bias_grad = keep
        b.heads_w_grad, b.heads_b_grad = o['heads_w'].ctypes.data, o['heads_b'].ctypes.data
        for k in ('h_pass', 'dxh', 'dz', 'dx', 'de', 'dh'):
            setattr(b, k, o[k].ctypes.data)
        b.scratch, b.enc_work = scratch.ctypes.data, work.ctypes.data
        o['chunks'] = check(lib.ic3_commnet_backward(env._h, C.byref(b), None))
        assert o['chunks'] == (T + tc - 1) // tc
        o['enc_dwt'], o['enc_db'] = nan(env.obs_dim, H), nan(H)
        if enc_window:
            fold = nan(lib.ic3_env_encode_backward_window_finish_scratch(env._h, H))
            check(lib.ic3_env_encode_backward_window_finish_ordered(env._h, H, p(o['enc_dwt']), p(o['enc_db']), p(work), p(fold), None))
        else:
            check(lib.ic3_env_encode_backward_finish(env._h, H, p(o['enc_dwt']), p(o['enc_db']), p(work), None))
        return o

    def errors(self, o, want):
        return ref.entry_errors(o, want, self.T, self.R)


ENTRY_CASES = [
    # name, env, H, P, T, mode_avg, comm_zero, gates, enc_window
    ('host_entry_pp', ('pp', (3, 6, 1, 'mixed', 5)), 64, 2, 3, True, False, True, 1),
    ('host_entry_tj', ('tj', (5, 6, 1, 'easy', 4)), 64, 1, 3, False, False, True, 1),
    ('host_entry_pp_zero', ('pp', (3, 6, 1, 'mixed', 4)), 64, 3, 2, True, True, False, 0),
]


def _env(spec):
    kind, cfg = spec
    if kind == 'pp':
        return HostEnv.pp(*cfg, seed=3)
    return HostEnv.tj(*cfg, seed=3, add_rate_min=0.6, add_rate_max=0.6)


@pytest.mark.parametrize("case,spec,H,P,T,mode_avg,comm_zero,gates,enc_window", ENTRY_CASES)
def test_commnet_backward_end_to_end_against_float64(case, spec, H, P, T, mode_avg, comm_zero, gates, enc_window):
    """ic3_commnet_backward over a window of T recorded states: the rings, every per-pass gradient (added onto what it held), the
    heads' and the encoder's gradient through the finish that goes with the form, against float64 from the dense observations."""
    env = _env(spec)
    try:
        w = ref.make_weights(29, H, P, 6, env.obs_dim)
        win = _Window(env, w, T, 41, mode_avg=mode_avg, comm_zero=comm_zero, gates=gates)
        o = win.run(enc_window=enc_window)
        assert o['chunks'] == 1
        ref.check(case, win.errors(o, win.reference()))
    finally:
        env.close()


def test_commnet_backward_chunks_against_one_chunk():
    """max_chunk_steps = 1 (T chunks of one step, the rings sized for one) against the window in one chunk: every gradient within the
    bar against float64, and the last chunk's rings bit-equal to the single chunk's rows of that step (rows are independent; only
    the sums over rows see the chunking)."""
    env = _env(('pp', (3, 6, 1, 'mixed', 5)))
    try:
        H, P, T = 64, 2, 3
        w = ref.make_weights(31, H, P, 6, env.obs_dim)
        win = _Window(env, w, T, 43)
        want = win.reference()
        one = win.run(max_chunk_steps=0)
        many = win.run(max_chunk_steps=1)
        assert one['chunks'] == 1 and many['chunks'] == T and many['tc'] == 1
        ref.check('host_chunks_one', win.errors(one, want))
        ref.check('host_chunks_many', win.errors(many, want))
        R = win.R
        for k in ('dz', 'dx', 'de', 'dh', 'dxh'):
            assert np.array_equal(many[k], one[k][(T - 1) * R:]), k
        assert np.array_equal(many['h_pass'], one['h_pass'][:, (T - 1) * R:])
        # two steps per chunk: a short last chunk
        two = win.run(max_chunk_steps=2)
        assert two['chunks'] == 2 and two['tc'] == 2
        ref.check('host_chunks_two', win.errors(two, want))
        assert np.array_equal(two['de'][:R], one['de'][(T - 1) * R:])
    finally:
        env.close()


def test_commnet_backward_struct_size_and_refusals():
    """ic3_commnet_backward reads struct_size first: -EINVAL before anything else is read (every pointer NULL here); a null handle /
    descriptor, T / E / N not the handle's, null buffers: -EINVAL; hid 32 / 96, 17 output columns: -ENOSYS; the queries answer 0
    where the call refuses."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    env = HostEnv.pp(10, 20, 1, 'mixed', 2, seed=1)
    tj = HostEnv.tj(10, 14, 1, 'medium', 2, seed=1)
    try:
        for e in (env, tj):
            for H in (64, 128, 256):
                assert lib.ic3_commnet_backward_supported(e._h, H, 10) == 1
                assert lib.ic3_commnet_backward_chunk_steps(e._h, 5, H, 0) == 5
                assert lib.ic3_commnet_backward_chunk_steps(e._h, 5, H, 2) == 2
                assert lib.ic3_commnet_backward_scratch_floats(e._h, 5, H, 0) > 0
            for H in (32, 96, 512):
                assert lib.ic3_commnet_backward_supported(e._h, H, 10) == 0
                assert lib.ic3_commnet_backward_chunk_steps(e._h, 5, H, 0) == 0
                assert lib.ic3_commnet_backward_scratch_floats(e._h, 5, H, 0) == 0
            assert lib.ic3_commnet_backward_supported(e._h, 128, 9) == 0          # not the handle's agents
        assert lib.ic3_commnet_backward_supported(None, 128, 10) == 0
        b = binding.CommnetBptt()
        b.struct_size = C.sizeof(b) - 8
        b.T, b.E, b.N, b.H, b.OT, b.passes = 4, 2, 10, 128, 6, 2
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -22
        assert b"ic3_commnet_bptt" in lib.ic3_last_error()
        b.struct_size = C.sizeof(b)
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -22        # (right size, null buffers)
        assert lib.ic3_commnet_backward(None, C.byref(b), None) == -22
        assert lib.ic3_commnet_backward(env._h, None, None) == -22
        b.E = 3
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -22        # (not the handle's E)
        b.E, b.H = 2, 32
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -38
        b.H = 96
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -38
        b.H, b.OT = 128, 17
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -38
        b.OT, b.passes = 6, 0
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -22
        b.passes, b.max_chunk_steps = 2, -1
        assert lib.ic3_commnet_backward(env._h, C.byref(b), None) == -22
    finally:
        env.close()
        tj.close()
