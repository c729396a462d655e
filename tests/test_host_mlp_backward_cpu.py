"""CPU: the IC baseline's (models.MLP) window backward (ic3_mlp_backward, csrc/bptt_kernels.hip) on the host build of the
product's own sources (tests/host/libic3rollout_host.so: the matrix-core kernel runs on the stand-in runtime) — the launch
(mlp_bwd_kernel) against float64, the sizes the library takes, and the struct_size handshake of ic3_mlp_bptt."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostEnv, check, host_lib, p


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _reference(e, h, dhead, w_heads, a2):
    """x1 = tanh(e); dz = (d . W_heads)(1 - h^2); de = (dz . A2 + dz)(1 - x1^2), in float64"""
    x1 = np.tanh(e.astype(np.float64))
    hv = h.astype(np.float64)
    dz = (dhead.astype(np.float64) @ w_heads.astype(np.float64)) * (1.0 - hv * hv)
    de = (dz @ a2.astype(np.float64) + dz) * (1.0 - x1 * x1)
    return x1, dz, de


@pytest.mark.parametrize("H,Q,OT", [(64, 70, 6), (128, 129, 16), (128, 64 * 5 + 3, 6)])
def test_mlp_step_against_float64(H, Q, OT):
    """ic3_mlp_backward_step, Q not a multiple of the 64-row tile: x1 written over e, dz, de and the bias partials against float64
    (the bars of the tanh-recurrence sibling: the same product length and arithmetic, fast_tanh within 2e-7); then accumulating
    onto the partials of the first call."""
    lib = host_lib()
    rng = np.random.default_rng(H * 1000 + Q)
    e = _f32(rng.standard_normal((Q, H)))
    h = _f32(np.tanh(rng.standard_normal((Q, H))))
    dhead, w_heads = _f32(rng.standard_normal((Q, OT))), _f32(rng.standard_normal((OT, H)) / H ** 0.5)
    a2 = _f32(rng.standard_normal((H, H)) / H ** 0.5)
    want_x1, want_dz, want_de = _reference(e, h, dhead, w_heads, a2)
    nparts = lib.ic3_mlp_backward_partials(Q, H)
    assert 1 <= nparts <= (Q + 63) // 64
    x1 = e.copy()
    dz = np.full((Q, H), np.nan, np.float32)
    de = np.full((Q, H), np.nan, np.float32)
    parts = np.full((nparts, H), np.nan, np.float32)
    n = check(lib.ic3_mlp_backward_step(p(x1), p(h), p(dhead), p(w_heads), OT, p(a2), p(dz), p(de), p(parts), 0, Q, H, None))
    assert n == nparts

    def compare():
        assert np.abs(x1 - want_x1).max() <= 2e-6 * max(1.0, np.abs(want_x1).max())
        assert np.abs(dz - want_dz).max() <= 2e-6 * max(1.0, np.abs(want_dz).max())
        assert np.abs(de - want_de).max() <= 4e-6 * max(1.0, np.abs(want_de).max())
    compare()
    np.testing.assert_allclose(parts.astype(np.float64).sum(0), want_dz.sum(0), rtol=1e-5, atol=1e-4)
    # accumulating onto the partials of the call before (e again in the in / out buffer)
    before = parts.astype(np.float64).sum(0)
    x1[:] = e
    dz[:] = np.nan
    de[:] = np.nan
    assert check(lib.ic3_mlp_backward_step(p(x1), p(h), p(dhead), p(w_heads), OT, p(a2), p(dz), p(de), p(parts), 1, Q, H,
                                           None)) == nparts
    compare()
    np.testing.assert_allclose(parts.astype(np.float64).sum(0), before + want_dz.sum(0), rtol=1e-5, atol=1e-4)


def test_mlp_backward_supported_sizes():
    """ic3_mlp_backward_supported: hid 64 / 128 on Predator-Prey and Traffic-Junction; not 32, 96 or 256 (those keep the loop); the
    partials query answers 0 where the launch refuses; the launch itself: -ENOSYS for another hid_size or more than 16 output
    columns, -EINVAL for a null buffer."""
    lib = host_lib()
    env = HostEnv.pp(10, 20, 1, 'mixed', 2, seed=1)
    tj = HostEnv.tj(10, 14, 1, 'medium', 2, seed=1)
    try:
        for e in (env, tj):
            assert lib.ic3_mlp_backward_supported(e._h, 64) == 1
            assert lib.ic3_mlp_backward_supported(e._h, 128) == 1
            for H in (32, 96, 256):
                assert lib.ic3_mlp_backward_supported(e._h, H) == 0
        assert lib.ic3_mlp_backward_supported(None, 128) == 0
    finally:
        env.close()
        tj.close()
    assert lib.ic3_mlp_backward_partials(100, 256) == 0
    assert lib.ic3_mlp_backward_partials(0, 128) == 0
    assert 1 <= lib.ic3_mlp_backward_partials(100, 128) <= 2
    assert lib.ic3_mlp_backward_partials(2 ** 33, 128) >= 1
    Q = 8
    buf = lambda *s: np.zeros(s, np.float32)
    for H, OT, want in ((32, 6, -38), (256, 6, -38), (128, 17, -38), (128, 0, -22)):
        x1, h, dz, de, parts = buf(Q, H), buf(Q, H), buf(Q, H), buf(Q, H), buf(1, H)
        d, w, a2 = buf(Q, max(OT, 1)), buf(max(OT, 1), H), buf(H, H)
        assert lib.ic3_mlp_backward_step(p(x1), p(h), p(d), p(w), OT, p(a2), p(dz), p(de), p(parts), 0, Q, H, None) == want
    x1, h = buf(Q, 64), buf(Q, 64)
    assert lib.ic3_mlp_backward_step(p(x1), p(h), None, None, 6, None, None, None, None, 0, Q, 64, None) == -22


def test_mlp_backward_rejects_a_wrong_struct_size():
    """ic3_mlp_backward reads struct_size first: a caller built against another layout gets -EINVAL before anything else is read
    (every pointer NULL here); a null handle / descriptor as well; hid 32 and 17 output columns: -ENOSYS."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    env = HostEnv.pp(10, 20, 1, 'mixed', 2, seed=1)
    try:
        b = binding.MlpBptt()
        b.struct_size = C.sizeof(b) - 8
        b.T, b.E, b.N, b.H, b.OT = 4, 2, 10, 128, 6
        assert lib.ic3_mlp_backward(env._h, C.byref(b), None) == -22
        assert b"ic3_mlp_bptt" in lib.ic3_last_error()
        b.struct_size = C.sizeof(b)
        assert lib.ic3_mlp_backward(env._h, C.byref(b), None) == -22        # (right size, null buffers)
        assert lib.ic3_mlp_backward(None, C.byref(b), None) == -22
        b.H = 32
        assert lib.ic3_mlp_backward(env._h, C.byref(b), None) == -38
        b.H, b.OT = 128, 17
        assert lib.ic3_mlp_backward(env._h, C.byref(b), None) == -38
    finally:
        env.close()


@pytest.mark.parametrize("kind,enc_window", [('pp', 1), ('pp', 0), ('tj', 1), ('tj', 0)])
def test_mlp_backward_end_to_end_against_float64(kind, enc_window):
    """ic3_mlp_backward over a window of T = 3 recorded states at hid 64: the x1 / dz / de rings, the partials' sum and a2_grad
    (added onto what it held) against float64 from the dense observations, then the encoder's gradient through the finish that
    goes with the form — the window form (its ordered and its plain finish) and the per-step form (enc_window = 0)."""
    from ic3net_amd import _lib as binding
    from test_host_abi_cpu import _play
    lib = host_lib()
    env = HostEnv.pp(3, 6, 1, 'mixed', 4, seed=3) if kind == 'pp' else \
        HostEnv.tj(5, 6, 1, 'easy', 4, seed=3, add_rate_min=0.6, add_rate_max=0.6)
    H, T, OT = 64, 3, 6
    R = env.E * env.N
    Q = T * R
    rng = np.random.default_rng(23)
    wt = _f32(rng.standard_normal((env.obs_dim, H)) * 0.3)
    b1 = _f32(rng.standard_normal(H) * 0.1)
    a2 = _f32(rng.standard_normal((H, H)) / H ** 0.5)
    w_heads = _f32(rng.standard_normal((OT, H)) / H ** 0.5)
    h = _f32(np.tanh(rng.standard_normal((T, R, H))))
    dhead = _f32(rng.standard_normal((T, R, OT)))
    snaps, obs = [], []
    for t in range(T):
        _play(env, 2 + t, 70 + t)
        snaps.append(env.snapshot())
        obs.append(env.observe().reshape(R, env.obs_dim).astype(np.float64))
    snaps = np.ascontiguousarray(np.stack(snaps))
    e = np.stack([o @ wt.astype(np.float64) + b1.astype(np.float64) for o in obs])
    want_x1, want_dz, want_de = _reference(e.reshape(Q, H), h.reshape(Q, H), dhead.reshape(Q, OT), w_heads, a2)
    x1, dz, de = (np.full((T, R, H), np.nan, np.float32) for _ in range(3))
    parts = np.full((lib.ic3_mlp_backward_partials(Q, H), H), np.nan, np.float32)
    n = int(lib.ic3_env_encode_backward_window_work(env._h, H) if enc_window else lib.ic3_env_encode_backward_work(env._h, H))
    assert n > 0
    work = np.full((n,), np.nan, np.float32)
    a2_grad = _f32(rng.standard_normal((H, H)))
    a2_before = a2_grad.astype(np.float64)
    scratch = np.zeros(lib.ic3_rnn_weight_grad_scratch_floats(Q, H), np.float32)
    b = binding.MlpBptt()
    b.struct_size = C.sizeof(b)
    b.T, b.E, b.N, b.H, b.OT = T, env.E, env.N, H, OT
    b.enc_first, b.enc_window = 1, enc_window
    b.h, b.dhead, b.snaps, b.snap_words = h.ctypes.data, dhead.ctypes.data, snaps.ctypes.data, snaps.shape[1]
    b.enc_wt, b.enc_bias, b.loc_table = wt.ctypes.data, b1.ctypes.data, None
    b.a2, b.w_heads = a2.ctypes.data, w_heads.ctypes.data
    b.x1, b.dz, b.de, b.dbias_partials = x1.ctypes.data, dz.ctypes.data, de.ctypes.data, parts.ctypes.data
    b.enc_work, b.a2_grad, b.wgrad_scratch = work.ctypes.data, a2_grad.ctypes.data, scratch.ctypes.data
    check(lib.ic3_mlp_backward(env._h, C.byref(b), None))
    assert np.abs(x1.reshape(Q, H) - want_x1).max() <= 2e-6 * max(1.0, np.abs(want_x1).max())
    assert np.abs(dz.reshape(Q, H) - want_dz).max() <= 2e-6 * max(1.0, np.abs(want_dz).max())
    assert np.abs(de.reshape(Q, H) - want_de).max() <= 4e-6 * max(1.0, np.abs(want_de).max())
    np.testing.assert_allclose(parts.astype(np.float64).sum(0), want_dz.sum(0), rtol=1e-5, atol=1e-4)
    want_a2 = a2_before + want_dz.T @ want_x1
    assert np.abs(a2_grad - want_a2).max() <= 4e-6 * max(1.0, np.abs(want_a2).max())
    want_w = sum(o.T @ want_de[t * R:(t + 1) * R] for t, o in enumerate(obs))
    want_b = want_de.sum(0)
    finishes = []
    if enc_window:
        fold = np.full((lib.ic3_env_encode_backward_window_finish_scratch(env._h, H),), np.nan, np.float32)
        finishes.append(lambda w_, b_: lib.ic3_env_encode_backward_window_finish_ordered(env._h, H, p(w_), p(b_), p(work), p(fold), None))
        finishes.append(lambda w_, b_: lib.ic3_env_encode_backward_window_finish(env._h, H, p(w_), p(b_), p(work), None))
    else:
        finishes.append(lambda w_, b_: lib.ic3_env_encode_backward_finish(env._h, H, p(w_), p(b_), p(work), None))
    for fin in finishes:
        dwt = np.full((env.obs_dim, H), np.nan, np.float32)
        db = np.full((H,), np.nan, np.float32)
        check(fin(dwt, db))
        np.testing.assert_allclose(dwt, want_w, rtol=0, atol=4e-5)       # (the encoder backward's bar at these sizes)
        np.testing.assert_allclose(db, want_b, rtol=0, atol=4e-5)
    env.close()
