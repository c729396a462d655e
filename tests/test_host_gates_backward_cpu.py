"""CPU: ic3_lstm_gates_backward_given at hid 64 / 128 — the launch ic3_bptt_backward issues per step and chain
(lstm_gates_bwd_kernel<64 | 128, 1, 1>) — on the host build of the product's own sources, in the forms the window uses: the
collection-mode cuts, dh / dc NULL (a detach point: read through an empty buffer descriptor), in place on the record, accumulating
bias partials, the heads' share at OT = 1 / 6 / 16 — against the float64 closed form (tests/bptt_window_ref.py).  The GPU twin is
tests/test_gates_backward_gpu.py::test_gates_backward_given_forms_of_the_window."""
import numpy as np
import pytest

import bptt_window_ref as ref
from host_abi_util import check, host_lib, p


@pytest.mark.parametrize("OT", [1, 6, 16])
@pytest.mark.parametrize("H,R", ref.GATE_SHAPES)
def test_gates_backward_given_forms_of_the_window(H, R, OT):
    """Every form of GATE_FORMS, in place (dgates over the gates, dc_prev over dc) and accumulating onto non-zero partial rows: dgates /
    dc_prev within 2e-6, dxh within 6e-6 (the bars of the launch's other tests), every partial row's increment; then the copy of
    h_prev times row_live into the h half of a wide xh."""
    lib = host_lib()
    s = ref.make_gate_step(1000 * H + 10 * R + OT, H, R, OT)
    wb3 = np.zeros(3 * 4 * H * 2 * H, np.uint16)
    check(lib.ic3_policy_pack_split_bwd(p(s['w_ih']), p(s['w_hh']), p(wb3), H, None))
    tiles = (R + 63) // 64
    # (the emulated matrix cores take ~0.7 s per 64-row tile at hid 128: the 10-tile shape walks the eight forms across its three OTs,
    #  the 71-tile shape runs ONE form per OT — every form runs at every hid-64 shape; the GPU twin runs the full product)
    k = [1, 6, 16].index(OT)
    if H == 64:
        forms = ref.GATE_FORMS
    elif R <= 640:
        forms = [f for j, f in enumerate(ref.GATE_FORMS) if j % 3 == k]
    else:
        forms = [ref.GATE_FORMS[(3, 1, 7)[k]]]
    for form in forms:
        want_dg, want_dc, want_dx, want_rows = ref.gate_step_reference(s, form)
        rec = s['gates'].copy()
        dc_io = s['dc'].copy() if form['dc'] else np.full((R, H), np.nan, np.float32)
        parts = s['parts0'].copy()
        dxh = np.full((R, 2 * H), np.nan, np.float32)
        n = check(lib.ic3_lstm_gates_backward_given(p(rec), None, 0, None, p(wb3), p(s['c_prev']), p(s['dh']) if form['dh'] else None,
                                                    p(dc_io) if form['dc'] else None, p(rec), p(dc_io), p(parts), 1, p(dxh),
                                                    p(s['live']) if form['cut'] else None,
                                                    p(s['keep']) if (form['cut'] and form['dc']) else None, p(s['dhead']),
                                                    p(s['w_heads']), OT, R, H, None))
        assert n == tiles, form
        assert np.abs(rec - want_dg).max() <= 2e-6 * max(1.0, np.abs(want_dg).max()), form
        assert np.abs(dc_io - want_dc).max() <= 2e-6 * max(1.0, np.abs(want_dc).max()), form
        assert np.abs(dxh - want_dx).max() <= 6e-6 * max(1.0, np.abs(want_dx).max()), form
        np.testing.assert_allclose(parts.astype(np.float64) - s['parts0'], want_rows, rtol=1e-5, atol=1e-4, err_msg=str(form))
    if OT == 1:
        xh = np.full((R, 2 * H + 4), np.nan, np.float32)
        dg, dcp = np.full((R, 4 * H), np.nan, np.float32), np.full((R, H), np.nan, np.float32)
        check(lib.ic3_lstm_gates_backward_given(p(s['gates']), p(xh), 2 * H + 4, p(s['h_prev']), None, p(s['c_prev']), p(s['dh']),
                                                p(s['dc']), p(dg), p(dcp), None, 0, None, p(s['live']), None, None, None, 0, R, H, None))
        np.testing.assert_array_equal(xh[:, H:2 * H], s['h_prev'] * s['live'][:, None])
        assert np.isnan(xh[:, :H]).all() and np.isnan(xh[:, 2 * H:]).all() and np.isfinite(dg).all()


def test_row_keep_without_dc_is_refused():
    """row_keep scales dc: with dc NULL the launch refuses (-EINVAL) — the combination ic3_bptt_backward now refuses up front."""
    lib = host_lib()
    s = ref.make_gate_step(1, 64, 8, 6)
    rec, dcp = s['gates'].copy(), np.zeros((8, 64), np.float32)
    assert lib.ic3_lstm_gates_backward_given(p(rec), None, 0, None, None, p(s['c_prev']), None, None, p(rec), p(dcp), None, 0, None, None,
                                             p(s['keep']), p(s['dhead']), p(s['w_heads']), 6, 8, 64, None) == -22
    assert b"row_keep" in lib.ic3_last_error()
    np.testing.assert_array_equal(rec, s['gates'])
