"""CPU: ic3_lstm_weight_grad_wide (csrc/bptt_kernels.hip compiled for the host, tests/host) — the LSTM cell's weight gradient of
a window at hid 256 against float64 in both arithmetics, the same bits as ic3_lstm_weight_grad at 64 / 128, its refusals, and
the K-slice plan that keeps a slice of config 5's window below the kernels' 32-bit buffer offsets."""
import numpy as np
import pytest

from host_abi_util import check, host_lib, p

f32 = lambda a: np.ascontiguousarray(a, np.float32)


def _operands(seed, Q, H, ldi):
    rng = np.random.default_rng(seed)
    inp, h, dg = f32(rng.standard_normal((Q, ldi))), f32(rng.standard_normal((Q, H))), f32(rng.standard_normal((Q, 4 * H)))
    return inp, h, dg, f32(rng.random(Q) < 0.8)


@pytest.mark.parametrize("Q,ldi", [(150, 256), (37, 512), (16, 256)])
def test_weight_gradient_at_hid_256_against_float64(Q, ldi):
    """dW (512, 1024) = [inp[:, :H] | live . h]^T . dgates, written into NaN-filled memory: the fp32 instruction and the nine exact
    bf16 products, with and without row_live, inp rows at stride H (the hid-256 record) and 2H; then accumulated onto itself.  The
    bar is the one of the entry's host test at 64 / 128 (test_host_policy_step_cpu.py), same row counts."""
    H = 256
    lib = host_lib()
    inp, h, dg, live = _operands(H + Q, Q, H, ldi)
    n = lib.ic3_lstm_weight_grad_wide_scratch_floats(Q, H, ldi)
    assert n > 0 and n % (2 * H * 4 * H) == 0
    scratch = np.full(n, np.nan, np.float32)
    before = dg.copy()
    for lv, split in ((None, 0), (live, 0), (None, 1), (live, 1)):
        x = np.concatenate([inp[:, :H].astype(np.float64), h.astype(np.float64) * (1.0 if lv is None else lv[:, None])], 1)
        want = x.T @ dg.astype(np.float64)
        dW = np.full((2 * H, 4 * H), np.nan, np.float32)
        ks = check(lib.ic3_lstm_weight_grad_wide(p(inp), ldi, p(h), p(dg), p(lv), Q, H, p(dW), 0, split, p(scratch), None))
        assert ks * 2 * H * 4 * H == n
        err = np.abs(dW - want).max()
        print("Q %d ldi %d split %d live %s: max err %.3g, max |want| %.3g" % (Q, ldi, split, lv is not None, err, np.abs(want).max()))
        assert err <= 2e-5 * max(1.0, np.abs(want).max())
        once = dW.copy()
        check(lib.ic3_lstm_weight_grad_wide(p(inp), ldi, p(h), p(dg), p(lv), Q, H, p(dW), 1, split, p(scratch), None))
        np.testing.assert_allclose(dW, 2 * once, rtol=1e-6)
    np.testing.assert_array_equal(dg, before)                    # (row_live scales the h rows on the way in: dgates is only read)


@pytest.mark.parametrize("H,Q,ldi", [(64, 200, 128), (128, 150, 256)])
def test_wide_entry_gives_the_bits_of_the_earlier_entry_at_64_and_128(H, Q, ldi):
    lib = host_lib()
    inp, h, dg, live = _operands(H + Q, Q, H, ldi)
    n = lib.ic3_lstm_weight_grad_scratch_floats(Q, H)
    assert n > 0 and lib.ic3_lstm_weight_grad_wide_scratch_floats(Q, H, ldi) == n
    for split in (0, 1):
        got = []
        for fn in (lib.ic3_lstm_weight_grad, lib.ic3_lstm_weight_grad_wide):
            scratch = np.full(n, np.nan, np.float32)
            dW = np.full((2 * H, 4 * H), np.nan, np.float32)
            got.append((check(fn(p(inp), ldi, p(h), p(dg), p(live), Q, H, p(dW), 0, split, p(scratch), None)), dW, scratch))
        assert got[0][0] == got[1][0]
        assert np.isfinite(got[0][1]).all()
        np.testing.assert_array_equal(got[0][1], got[1][1])
        np.testing.assert_array_equal(got[0][2], got[1][2])      # (every partial, not only their sum)


def test_refusals_of_the_wide_entry():
    lib = host_lib()
    H, Q = 256, 16
    inp, h, dg, _ = _operands(1, Q, H, H)
    n = lib.ic3_lstm_weight_grad_wide_scratch_floats(Q, H, H)
    scratch, dW = np.zeros(n, np.float32), np.zeros((2 * H, 4 * H), np.float32)
    assert lib.ic3_lstm_weight_grad_wide(p(inp), H - 4, p(h), p(dg), None, Q, H, p(dW), 0, 0, p(scratch), None) == -22
    assert lib.ic3_lstm_weight_grad_wide(p(inp), 96, p(h), p(dg), None, Q, 96, p(dW), 0, 0, p(scratch), None) == -38
    assert lib.ic3_lstm_weight_grad_wide_scratch_floats(Q, 96, 96) == 0
    assert lib.ic3_lstm_weight_grad_scratch_floats(Q, 256) == 0  # (the earlier pair keeps its contract)
    assert lib.ic3_lstm_weight_grad(p(inp), H, p(h), p(dg), None, Q, H, p(dW), 0, 0, p(scratch), None) == -38
    assert not dW.any()


def _plan_holds(lib):
    """ks as the scratch query derives it (the call derives the same): a K slice of config 5's 80-step window at E = 8192 stays
    below 2^31 bytes per operand, whatever inp's row stride; a short window gets no slice under one 16-row stage."""
    H = 256
    one = 2 * H * 4 * H
    Q = 80 * 8192 * 32
    for ldi in (256, 1024):
        n = lib.ic3_lstm_weight_grad_wide_scratch_floats(Q, H, ldi)
        assert n > 0 and n % one == 0
        ks = n // one
        per = -(-(-(-Q // ks)) // 16) * 16
        print("ldi %d: ks %d, %d rows per slice, %.3f GB per operand" % (ldi, ks, per, per * max(ldi, 4 * H) * 4 / 2 ** 30))
        assert per * max(ldi, 4 * H) * 4 < 2 ** 31
    n = lib.ic3_lstm_weight_grad_wide_scratch_floats(150, H, 256)
    assert n > 0 and n % one == 0 and n // one <= -(-150 // 16)


def test_slice_plan_at_hid_256_host_library():
    _plan_holds(host_lib())


def test_slice_plan_at_hid_256_gpu_library():
    """The plan is a host function: the product's own library answers without a device (256 CUs assumed then)."""
    from ic3net_amd import _lib
    _plan_holds(_lib.lib())
