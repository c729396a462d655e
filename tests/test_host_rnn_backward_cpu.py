"""CPU: the tanh-recurrence baseline's window backward (ic3_rnn_backward, csrc/bptt_kernels.hip) on the host build of the
product's own sources (tests/host/libic3rollout_host.so: the matrix-core kernels run on the stand-in runtime) — the per-step launch
(rnn_tanh_bwd_kernel) and affine2's window weight gradient (rnn_wgrad_kernel) against float64, the sizes the library takes, and
the struct_size handshake of ic3_rnn_bptt."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostEnv, check, host_lib, p


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _step_reference(dh_in, h, dhead, w_heads, a2, scale):
    dh = (0.0 if dh_in is None else dh_in.astype(np.float64)) + dhead.astype(np.float64) @ w_heads.astype(np.float64)
    hv = h.astype(np.float64)
    dz = dh * (1.0 - hv * hv)
    out = dz @ a2.astype(np.float64)
    if scale is not None:
        out = out * scale.astype(np.float64)[:, None]
    return dz, out


@pytest.mark.parametrize("H,R,OT", [(64, 70, 6), (128, 129, 16), (128, 64 * 5 + 3, 6), (64, 200, 16)])
def test_tanh_step_against_float64(H, R, OT):
    """ic3_rnn_tanh_backward_step, R not a multiple of the 64-row tile: dz = (dh_in + d . W_heads)(1 - h^2), dh_out = (dz . A2) *
    row_keep, the bias partials; with and without the cut, with a detach point (dh_in NULL), in place (dh_out = dh_in), and
    accumulating partials."""
    lib = host_lib()
    rng = np.random.default_rng(H * 1000 + R)
    h = _f32(np.tanh(rng.standard_normal((R, H))))
    dh_in = _f32(rng.standard_normal((R, H)))
    dhead, w_heads = _f32(rng.standard_normal((R, OT))), _f32(rng.standard_normal((OT, H)) / H ** 0.5)
    a2 = _f32(rng.standard_normal((H, H)) / H ** 0.5)
    keep = _f32(rng.random(R) < 0.6)
    nparts = lib.ic3_rnn_backward_partials(R, H)
    assert 1 <= nparts <= (R + 63) // 64
    for cut, detached in ((False, False), (True, False), (False, True)):
        want_dz, want_out = _step_reference(None if detached else dh_in, h, dhead, w_heads, a2, keep if cut else None)
        dz = np.full((R, H), np.nan, np.float32)
        out = np.full((R, H), np.nan, np.float32)
        parts = np.full((nparts, H), np.nan, np.float32)
        n = check(lib.ic3_rnn_tanh_backward_step(None if detached else p(dh_in), p(h), p(dhead), p(w_heads), OT, p(a2),
                                                 p(keep) if cut else None, p(dz), p(out), p(parts), 0, R, H, None))
        assert n == nparts
        assert np.abs(dz - want_dz).max() <= 2e-6 * max(1.0, np.abs(want_dz).max())
        assert np.abs(out - want_out).max() <= 4e-6 * max(1.0, np.abs(want_out).max())
        np.testing.assert_allclose(parts.astype(np.float64).sum(0), want_dz.sum(0), rtol=1e-5, atol=1e-4)
    # in place (the chain hands dh_out to the next step in the same buffer), partials accumulated on top of the last ones
    want_dz, want_out = _step_reference(dh_in, h, dhead, w_heads, a2, keep)
    before = parts.astype(np.float64).sum(0)
    buf = dh_in.copy()
    check(lib.ic3_rnn_tanh_backward_step(p(buf), p(h), p(dhead), p(w_heads), OT, p(a2), p(keep), p(dz), p(buf), p(parts), 1, R, H,
                                         None))
    assert np.abs(buf - want_out).max() <= 4e-6 * max(1.0, np.abs(want_out).max())
    np.testing.assert_allclose(parts.astype(np.float64).sum(0), before + want_dz.sum(0), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("H,Q", [(64, 1000), (128, 16 * 37 + 5), (128, 3)])
def test_window_weight_grad_against_float64(H, Q):
    """ic3_rnn_weight_grad at a ragged Q (not a multiple of the 16-row stage, nor of the K slices): dA2 = dz^T (row_live h_prev),
    written, then accumulated; without row_live too."""
    lib = host_lib()
    rng = np.random.default_rng(Q + H)
    dz, hp = _f32(rng.standard_normal((Q, H))), _f32(rng.standard_normal((Q, H)))
    live = _f32(rng.random(Q) < 0.7)
    scratch = np.zeros(lib.ic3_rnn_weight_grad_scratch_floats(Q, H), np.float32)
    for lv in (live, None):
        hv = hp.astype(np.float64) * (lv[:, None] if lv is not None else 1.0)
        want = dz.astype(np.float64).T @ hv
        dA = np.full((H, H), np.nan, np.float32)
        check(lib.ic3_rnn_weight_grad(p(dz), p(hp), p(lv), Q, H, p(dA), 0, p(scratch), None))
        assert np.abs(dA - want).max() <= 2e-6 * max(1.0, np.abs(want).max()) * max(1.0, Q ** 0.5 / 8)
        check(lib.ic3_rnn_weight_grad(p(dz), p(hp), p(lv), Q, H, p(dA), 1, p(scratch), None))
        assert np.abs(dA - 2 * want).max() <= 4e-6 * max(1.0, np.abs(want).max()) * max(1.0, Q ** 0.5 / 8)


def test_rnn_backward_supported_sizes():
    """ic3_rnn_backward_supported: hid 64 / 128 on Predator-Prey and Traffic-Junction; not 32, 96 or 256 (those keep the loop);
    the scratch queries answer 0 where the launches refuse."""
    lib = host_lib()
    env = HostEnv.pp(10, 20, 1, 'mixed', 2, seed=1)
    tj = HostEnv.tj(10, 14, 1, 'medium', 2, seed=1)
    try:
        for e in (env, tj):
            assert lib.ic3_rnn_backward_supported(e._h, 64) == 1
            assert lib.ic3_rnn_backward_supported(e._h, 128) == 1
            for H in (32, 96, 256):
                assert lib.ic3_rnn_backward_supported(e._h, H) == 0
        assert lib.ic3_rnn_backward_supported(None, 128) == 0
    finally:
        env.close()
        tj.close()
    assert lib.ic3_rnn_weight_grad_scratch_floats(100, 256) == 0
    assert lib.ic3_rnn_backward_partials(100, 256) == 0
    assert lib.ic3_rnn_backward_partials(100, 128) >= 1


def test_rnn_backward_rejects_a_wrong_struct_size():
    """ic3_rnn_backward reads struct_size first: a caller built against another layout gets -EINVAL before anything else is read
    (every pointer NULL here); a null handle / descriptor as well."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    env = HostEnv.pp(10, 20, 1, 'mixed', 2, seed=1)
    try:
        b = binding.RnnBptt()
        b.struct_size = C.sizeof(b) - 8
        b.T, b.E, b.N, b.H, b.OT = 4, 2, 10, 128, 6
        assert lib.ic3_rnn_backward(env._h, C.byref(b), None) == -22
        assert b"ic3_rnn_bptt" in lib.ic3_last_error()
        b.struct_size = C.sizeof(b)
        assert lib.ic3_rnn_backward(env._h, C.byref(b), None) == -22        # (right size, null buffers)
        assert lib.ic3_rnn_backward(None, C.byref(b), None) == -22
    finally:
        env.close()
