"""CPU: the pieces of the window backward (ic3_bptt_backward) at hid 256 on the host build of the product's own sources
(tests/host/libic3rollout_host.so: the matrix-core kernels run on the stand-in runtime) — the recorded-gates cell derivative and
its input gradient (lstm_gates_bwd_kernel<256, 1, 1>), the communication backward (comm_bwd_kernel<256>), the step launch's gate
record at 256 (inp rows of stride H) and the window's weight-gradient products, against float64."""
import numpy as np
import pytest

from host_abi_util import HostEnv, HostPolicy, check, host_lib, p

H = 256


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def test_bptt_backward_supported_at_hid_256():
    """ic3_bptt_backward_supported: hid 256 on the config-5 grid (32 agents, dim 40, vision 2) and on Traffic-Junction — not
    beyond 256, nor for more than 64 agents."""
    lib = host_lib()
    env = HostEnv.pp(32, 40, 2, 'mixed', 2, seed=1)
    tj = HostEnv.tj(20, 18, 1, 'hard', 2, seed=1)
    try:
        assert lib.ic3_bptt_backward_supported(env._h, 256) == 1
        assert lib.ic3_bptt_backward_supported(tj._h, 256) == 1
        assert lib.ic3_bptt_backward_supported(env._h, 512) == 0
    finally:
        env.close()
        tj.close()


@pytest.mark.parametrize("R", [70, 129])
def test_gates_backward_given_at_hid_256(R):
    """ic3_lstm_gates_backward_given at hid 256 (R not a multiple of 64: a ragged last tile): the cell's derivative of the
    recorded gates, the heads' share folded into dL/dh, [d inp | d h_prev] = dgates . [W_ih | W_hh] on the split planes, the
    collection-mode cuts and the bias partials — against float64; in place on the record as ic3_bptt_backward runs it."""
    lib = host_lib()
    rng = np.random.default_rng(R)
    w_ih, w_hh = _f32(rng.standard_normal((4 * H, H)) / H ** 0.5), _f32(rng.standard_normal((4 * H, H)) / H ** 0.5)
    wb3 = np.zeros(3 * 4 * H * 2 * H, np.uint16)
    check(lib.ic3_policy_pack_split_bwd(p(w_ih), p(w_hh), p(wb3), H, None))
    sig = lambda z: 1 / (1 + np.exp(-z))
    pre = rng.standard_normal((R, 4 * H))
    acts = _f32(np.concatenate([sig(pre[:, :H]), sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])], 1))
    c_prev, dh, dc = [_f32(rng.standard_normal((R, H))) for _ in range(3)]
    OT = 8
    dhead, w_heads = _f32(rng.standard_normal((R, OT))), _f32(rng.standard_normal((OT, H)) / H ** 0.5)
    live = _f32(rng.random(R) < 0.7)
    keep = _f32(rng.random(R) < 0.6)
    tiles = (R + 63) // 64
    a = acts.astype(np.float64)
    ai, af, ag, ao = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    for cut in (False, True):
        cp = c_prev.astype(np.float64) * (live[:, None] if cut else 1.0)
        dcv = dc.astype(np.float64) * (keep[:, None] if cut else 1.0)
        dhv = dh.astype(np.float64) + dhead.astype(np.float64) @ w_heads.astype(np.float64)
        tc = np.tanh(af * cp + ai * ag)
        dct = dcv + dhv * ao * (1 - tc * tc)
        want = np.concatenate([dct * ag * ai * (1 - ai), dct * cp * af * (1 - af), dct * ai * (1 - ag * ag), dhv * tc * ao * (1 - ao)], 1)
        rec = acts.copy()                                        # dgates over the gates, as the window loop runs it
        dcp = np.full((R, H), np.nan, np.float32)
        dxh = np.full((R, 2 * H), np.nan, np.float32)
        parts = np.full((tiles, 4 * H), np.nan, np.float32)
        n = check(lib.ic3_lstm_gates_backward_given(p(rec), None, 0, None, p(wb3), p(c_prev), p(dh), p(dc), p(rec), p(dcp), p(parts), 0,
                                                    p(dxh), p(live) if cut else None, p(keep) if cut else None, p(dhead), p(w_heads),
                                                    OT, R, H, None))
        assert n == tiles
        assert np.abs(rec - want).max() <= 3e-6 * max(1.0, np.abs(want).max())
        assert np.abs(dcp - dct * af).max() <= 3e-6 * max(1.0, np.abs(dct * af).max())
        np.testing.assert_allclose(parts.astype(np.float64).sum(0), want.sum(0), rtol=1e-5, atol=1e-4)
        want_dx = rec.astype(np.float64) @ np.concatenate([w_ih, w_hh], 1).astype(np.float64)
        assert np.abs(dxh - want_dx).max() <= 6e-6 * max(1.0, np.abs(want_dx).max())
    # the copy of h_prev (times row_live) into the h half of a wide [inp | h] buffer works at 256 as well
    h_prev = _f32(rng.standard_normal((R, H)))
    xh = np.full((R, 2 * H), np.nan, np.float32)
    dg = np.full((R, 4 * H), np.nan, np.float32)
    check(lib.ic3_lstm_gates_backward_given(p(acts), p(xh), 2 * H, p(h_prev), None, p(c_prev), p(dh), p(dc), p(dg), p(dcp), None, 0,
                                            None, p(live), None, None, None, 0, R, H, None))
    np.testing.assert_array_equal(xh[:, H:], h_prev * live[:, None])
    assert np.isnan(xh[:, :H]).all()


def _mix(x, alive, gate, mode_avg):
    """comm.py:181-205 in closed form on (E, N, H) float64 (ic3_comm_masked_mean)."""
    E, N, _ = x.shape
    al = np.ones((E, N)) if alive is None else alive.astype(np.float64)
    g = al * (np.ones((E, N)) if gate is None else gate.astype(np.float64))
    S = (g[:, :, None] * x).sum(1, keepdims=True)
    n_alive = al.sum(1)
    scale = np.where(n_alive > 1, 1.0 / np.maximum(n_alive - 1, 1), 1.0) if mode_avg else np.ones(E)
    return g[:, :, None] * (S - g[:, :, None] * x) * scale[:, None, None]


@pytest.mark.parametrize("N,E,avg", [(32, 5, True), (64, 3, False), (32, 4, False)])
def test_comm_backward_at_hid_256(N, E, avg):
    """ic3_comm_backward at hid 256 with dead and gated-off agents: dh_out = (d h_direct + (M d inp) . C) * out_scale and the
    partials of (M d inp)^T . h_prev against float64; written, then accumulated."""
    lib = host_lib()
    rng = np.random.default_rng(N + E)
    R = E * N
    dxh, hp = _f32(rng.standard_normal((R, 2 * H))), _f32(rng.standard_normal((R, H)))
    cw = _f32(rng.standard_normal((H, H)) / H ** 0.5)
    alive = (rng.random((E, N)) < 0.8).astype(np.int32)
    gate = (rng.random((E, N)) < 0.6).astype(np.int32)
    alive[0, :] = 0                                              # an env with nobody alive
    alive[1, 1:] = 0                                             # ... and one with a single agent alive
    scale = _f32(rng.random(R) < 0.7)
    dinp, dhd = dxh[:, :H].astype(np.float64), dxh[:, H:].astype(np.float64)
    want_dh = (dhd + _mix((dinp @ cw.astype(np.float64)).reshape(E, N, H), alive, gate, avg).reshape(R, H)) * scale[:, None]
    want_dc = dinp.T @ _mix(hp.astype(np.float64).reshape(E, N, H), alive, gate, avg).reshape(R, H)
    nparts = lib.ic3_comm_backward_partials(E, N)
    dh = np.full((R, H), np.nan, np.float32)
    parts = np.full((nparts, H, H), np.nan, np.float32)
    n = check(lib.ic3_comm_backward(p(dxh), 2 * H, p(hp), p(alive), p(gate), p(cw), p(scale), p(dh), p(parts), 0, E, N, H, int(avg), 0,
                                    None))
    assert n == nparts
    assert np.abs(dh - want_dh).max() <= 4e-6 * max(1.0, np.abs(want_dh).max())
    assert np.abs(parts.astype(np.float64).sum(0) - want_dc).max() <= 1e-5 * max(1.0, np.abs(want_dc).max())
    before = parts.copy()
    check(lib.ic3_comm_backward(p(dxh), 2 * H, p(hp), p(alive), p(gate), p(cw), None, p(dh), p(parts), 1, E, N, H, int(avg), 0, None))
    np.testing.assert_allclose(parts, 2 * before, rtol=1e-6, atol=1e-6)


def test_gate_record_at_hid_256():
    """ic3_env_set_record_out at hid 256 (config-5 grid: 32 agents, dim 40, vision 2): every output of the step launch the
    same bits armed or not; the activated gates reproduce (c', h'); the inp rows are stored at row stride H and, with the
    state that entered, reproduce the gates."""
    from test_host_policy_step_cpu import WORKLOADS, make_env, make_params
    w = WORKLOADS['pp_scaled']
    E, N, heads = 2, w['N'], w['heads']
    res = []
    for armed in (False, True):
        env = make_env(w, E, 3, 70)
        P = make_params(env.obs_dim, H, heads, seed=4)
        pol = HostPolicy(env, P, H, heads, gate_split=True)
        env.reset()
        rng = np.random.default_rng(1)
        h = (rng.standard_normal((E * N, H)) * 0.3).astype(np.float32)
        c = (rng.standard_normal((E * N, H)) * 0.3).astype(np.float32)
        h0, c0 = h.copy(), c.copy()
        gate = np.ones((E, N), np.int32)
        gates = np.full((E * N, 4 * H), np.nan, np.float32)
        xrows = np.full((E * N + 1, H), np.nan, np.float32)      # (one row past the record: must stay untouched)
        if armed:
            check(env.lib.ic3_env_set_record_out(env._h, p(gates), p(xrows)))
        out, act, obs, rew, done, alive, comp = pol.step(env, h, c, None, gate)
        res.append((h.copy(), c.copy(), out.copy(), act.copy(), obs.copy(), rew.copy()))
        if armed:
            assert np.isfinite(gates).all() and np.isfinite(xrows[:E * N]).all() and np.isnan(xrows[E * N]).all()
            g64 = gates.astype(np.float64)
            gi, gf, gg, go = g64[:, :H], g64[:, H:2 * H], g64[:, 2 * H:3 * H], g64[:, 3 * H:]
            c1 = gf * c0 + gi * gg
            assert np.abs(c1 - c).max() <= 1e-6
            assert np.abs(go * np.tanh(c1) - h).max() <= 2e-6
            pre = np.concatenate([xrows[:E * N], h0], 1).astype(np.float64) @ \
                np.concatenate([pol.w_ih, pol.w_hh], 1).T.astype(np.float64) + (P['f_module.bias_ih'] + P['f_module.bias_hh'])
            # (1e-5: a K = 2H = 512 product in fp32 against float64 — hid 128's test has 2e-6 at half the K)
            assert np.abs(1 / (1 + np.exp(-pre[:, :H])) - gi).max() <= 1e-5
            assert np.abs(np.tanh(pre[:, 2 * H:3 * H]) - gg).max() <= 1e-5
        env.close()
    for x, y in zip(*res):
        np.testing.assert_array_equal(x, y)


def test_weight_gradient_products_at_hid_256():
    """bptt._weight_grad_products: the window's [W_ih | W_hh] gradient at hid 256 over all T x R rows at once, inp^T . dgates and
    (row_live h)^T . dgates, added to dW — against float64 (CPU tensors: the same torch calls as on the device)."""
    import torch
    from types import SimpleNamespace
    from ic3net_amd import bptt
    T, R = 3, 50
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)
    rec = SimpleNamespace(xh=rn(T + 1, R, H), hs=rn(T + 1, R, H), gates=rn(T + 1, R, 4 * H))
    live = (torch.rand(T, R, generator=g) < 0.7).float()
    for lv in (None, live):
        dg = rec.gates[:T].double().reshape(T * R, 4 * H)
        x = torch.cat([rec.xh[:T].double().reshape(T * R, H),
                       rec.hs[:T].double().reshape(T * R, H) * (1.0 if lv is None else lv.double().reshape(T * R, 1))], 1)
        base = rn(2 * H, 4 * H)
        want = base.double() + x.t() @ dg
        dW = base.clone()
        gates = rec.gates.clone()
        bptt._weight_grad_products(SimpleNamespace(xh=rec.xh, hs=rec.hs, gates=gates), T, R, H, dW, lv)
        assert float((dW.double() - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))


def test_heads_gradient_without_a_side_stream_runs_behind_a_body_that_succeeded():
    """bptt._heads_grad_beside on CPU tensors (nothing to fork onto): the heads' pass runs on the way out of the `with` body — and
    not at all when the body raised."""
    import torch
    from types import SimpleNamespace
    from ic3net_amd import bptt
    T, R, Hh, OT = 3, 10, 8, 17                                  # (more than 16 columns: the library products, no HIP launch)
    g = torch.Generator().manual_seed(3)
    rec = bptt.EpisodeRecord(T, R, Hh, 1, 'cpu')
    rec.hs.copy_(torch.randn(T + 1, R, Hh, generator=g))
    rec.n, rec.h_last = T, rec.hs[T]
    d_out = torch.randn(T, R, OT, generator=g)
    acc = dict(w_heads=torch.zeros(OT, Hh), b_heads=torch.zeros(OT))
    with pytest.raises(ZeroDivisionError):
        with bptt._heads_grad_beside(SimpleNamespace(), rec, d_out, acc, T, R, Hh):
            1 // 0
    assert not acc['w_heads'].any() and not acc['b_heads'].any()
    with bptt._heads_grad_beside(SimpleNamespace(), rec, d_out, acc, T, R, Hh):
        assert not acc['w_heads'].any()
    want = d_out.double().reshape(T * R, OT).t() @ rec.hs[1:].double().reshape(T * R, Hh)
    assert float((acc['w_heads'].double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert float((acc['b_heads'].double() - d_out.double().sum((0, 1))).abs().max()) <= 1e-5 * T * R
