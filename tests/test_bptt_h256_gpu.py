"""GPU: the update half's window backward (ic3_bptt_backward, bptt._backward_window_native) at hid 256 — its kernels against
float64, the step launch's gate record at 256, and the gradients of whole updates (config 5's grid, a padded hid 200) against
the recomputing backward (args.record_gates=False) and against autograd through the rollout replaying the same actions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 256


def _rn(gen, *s):
    return torch.randn(*s, device='cuda', generator=gen)


def test_window_backward_supported_at_hid_256():
    """ops.bptt_backward_supported: hid 256 on the config-5 env (32 agents, dim 40, vision 2) and on Traffic-Junction."""
    import bench
    from ic3net_amd import ops
    tr, _ = bench.build_trainer('pp_scaled', 4, 3, 0, 0)
    assert ops.bptt_backward_supported(tr.env.env, 256)
    tj, _ = bench.build_trainer('tj_hard', 4, 3, 0, 0, hid_size=256)
    assert ops.bptt_backward_supported(tj.env.env, 256)


@pytest.mark.parametrize("R", [333, 64 * 70 + 17])
def test_given_gate_backward_at_hid_256_against_float64(R):
    """ops.lstm_gates_backward_given at hid 256, R not a multiple of 64: the cell's derivative of recorded gates, the heads' share
    folded in, the collection-mode cuts, [d inp | d h_prev] = dgates . [W_ih | W_hh] on the split planes, the bias partials."""
    from ic3net_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(R)
    w_ih, w_hh = _rn(gen, 4 * H, H) / H ** 0.5, _rn(gen, 4 * H, H) / H ** 0.5
    wb3 = ops.policy_pack_split_bwd(w_ih, w_hh)
    pre = _rn(gen, R, 4 * H)
    acts = torch.cat([torch.sigmoid(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])], 1).contiguous()
    c_prev, dh, dc = _rn(gen, R, H), _rn(gen, R, H), _rn(gen, R, H)
    OT = 16
    dhead, w_heads = _rn(gen, R, OT), _rn(gen, OT, H) / H ** 0.5
    live = (torch.rand(R, device='cuda', generator=gen) < 0.7).float()
    keep = (torch.rand(R, device='cuda', generator=gen) < 0.6).float()
    tiles = (R + 63) // 64
    a = acts.double()
    ai, af, ag, ao = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    for cut in (False, True):
        cp = c_prev.double() * (live[:, None].double() if cut else 1.0)
        dcv = dc.double() * (keep[:, None].double() if cut else 1.0)
        dhv = dh.double() + dhead.double() @ w_heads.double()
        tc = torch.tanh(af * cp + ai * ag)
        dct = dcv + dhv * ao * (1 - tc * tc)
        want = torch.cat([dct * ag * ai * (1 - ai), dct * cp * af * (1 - af), dct * ai * (1 - ag * ag), dhv * tc * ao * (1 - ao)], 1)
        rec = acts.clone()                                       # in place: dgates over the gates
        dcp = torch.full((R, H), float('nan'), device='cuda')
        dxh = torch.full((R, 2 * H), float('nan'), device='cuda')
        parts = torch.full((tiles, 4 * H), float('nan'), device='cuda')
        n = ops.lstm_gates_backward_given(rec, c_prev, dh, dc, rec, dcp, parts, False, lstm_wp3_bwd=wb3, dxh=dxh,
                                          row_live=live if cut else None, row_keep=keep if cut else None, dhead=dhead, w_heads=w_heads)
        assert n == tiles
        assert float((rec.double() - want).abs().max()) <= 3e-6 * max(1.0, float(want.abs().max()))
        assert float((dcp.double() - dct * af).abs().max()) <= 3e-6 * max(1.0, float((dct * af).abs().max()))
        torch.testing.assert_close(parts.double().sum(0), want.sum(0), atol=1e-4, rtol=1e-5)
        want_dx = rec.double() @ torch.cat([w_ih, w_hh], 1).double()
        assert float((dxh.double() - want_dx).abs().max()) <= 6e-6 * max(1.0, float(want_dx.abs().max()))


def _mix(x, alive, gate, mode_avg):
    """comm.py:181-205 in closed form on (E, N, H) float64."""
    al = alive.double()
    g = al * gate.double()
    S = (g[:, :, None] * x).sum(1, keepdim=True)
    n_alive = al.sum(1)
    scale = torch.where(n_alive > 1, 1.0 / torch.clamp(n_alive - 1, min=1), torch.ones_like(n_alive)) if mode_avg \
        else torch.ones_like(n_alive)
    return g[:, :, None] * (S - g[:, :, None] * x) * scale[:, None, None]


@pytest.mark.parametrize("N,E,avg", [(32, 301, True), (32, 40, False), (64, 37, True), (64, 9, False)])
def test_comm_backward_at_hid_256_against_float64(N, E, avg):
    """ops.comm_backward at hid 256 with dead and gated-off agents, N = 32 / 64, avg / sum, a row scale (collection mode); E = 301
    at N = 32: 151 tiles of two envs on the persistent grid."""
    from ic3net_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(N * E)
    R = E * N
    dxh, hp = _rn(gen, R, 2 * H), _rn(gen, R, H)
    cw = _rn(gen, H, H) / H ** 0.5
    alive = (torch.rand(E, N, device='cuda', generator=gen) < 0.8).int()
    gate = (torch.rand(E, N, device='cuda', generator=gen) < 0.6).int()
    alive[0] = 0
    alive[1, 1:] = 0
    scale = (torch.rand(R, device='cuda', generator=gen) < 0.7).float()
    dinp, dhd = dxh[:, :H].double(), dxh[:, H:].double()
    want_dh = (dhd + _mix((dinp @ cw.double()).view(E, N, H), alive, gate, avg).view(R, H)) * scale[:, None].double()
    want_dc = dinp.t() @ _mix(hp.double().view(E, N, H), alive, gate, avg).view(R, H)
    parts = torch.full((ops.comm_backward_partials(E, N), H, H), float('nan'), device='cuda')
    dh = torch.full((R, H), float('nan'), device='cuda')
    ops.comm_backward(dxh, hp, alive, gate, cw, dh, parts, E, N, mode_avg=avg, out_scale=scale, accumulate=False)
    assert float((dh.double() - want_dh).abs().max()) <= 4e-6 * max(1.0, float(want_dh.abs().max()))
    assert float((parts.double().sum(0) - want_dc).abs().max()) <= 1e-5 * max(1.0, float(want_dc.abs().max()))


def test_weight_gradient_products_at_hid_256_against_float64():
    """bptt._weight_grad_products on the device: inp^T . dgates and (row_live h)^T . dgates over T x R rows, added to dW."""
    from types import SimpleNamespace
    from ic3net_amd import bptt
    gen = torch.Generator(device='cuda').manual_seed(5)
    T, R = 4, 3000
    xh, hs, gates = _rn(gen, T + 1, R, H), _rn(gen, T + 1, R, H), _rn(gen, T + 1, R, 4 * H)
    live = (torch.rand(T, R, device='cuda', generator=gen) < 0.7).float()
    for lv in (None, live):
        x = torch.cat([xh[:T].double().reshape(T * R, H),
                       hs[:T].double().reshape(T * R, H) * (1.0 if lv is None else lv.double().reshape(T * R, 1))], 1)
        base = _rn(gen, 2 * H, 4 * H)
        want = base.double() + x.t() @ gates[:T].double().reshape(T * R, 4 * H)
        dW = base.clone()
        bptt._weight_grad_products(SimpleNamespace(xh=xh, hs=hs, gates=gates.clone()), T, R, H, dW, lv)
        assert float((dW.double() - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))


def _update(wl, E, T, record=True, collect=False, two=True, spy=None, **over):
    """One recorded batch through Trainer.run_batch + compute_grad_native; returns (grads, record of the first episode)."""
    import bench
    from ic3net_amd import ops
    tr, a = bench.build_trainer(wl, E, 3, 0, 0, **over)
    a.max_steps, a.batch_size = T, E * T * (2 if collect else 1)
    a.detach_gap = 3
    a.entr, a.value_coeff, a.gamma, a.normalize_rewards, a.advantages_per_action = 0.01, 0.01, 0.9, False, False
    a.record_gates, a.auto_reset, a.bptt_two_chains = record, collect, two
    assert tr._native_update()
    tr._records = []
    batch, _ = tr.run_batch(0)
    recs = tr._records
    rec = dict(n=recs[0].n, gates=recs[0].gates is not None and recs[0].gates_n == recs[0].n,
               hs=torch.cat([r.hs[:r.n] for r in recs]).clone(), cs=torch.cat([r.cs[:r.n] for r in recs]).clone())
    if rec['gates']:
        r0 = recs[0]
        rec.update(g=r0.gates[:r0.n].clone(), xh=r0.xh[:r0.n].clone(), knet=tr._kernel_net())
    calls = []
    orig = ops.bptt_backward

    def counting(*args, **kw):
        calls.append(args[4])                                    # (H)
        return orig(*args, **kw)
    ops.bptt_backward = counting
    try:
        tr.optimizer.zero_grad()
        tr.compute_grad_native(batch, recs)
    finally:
        ops.bptt_backward = orig
        tr._records = None
    torch.cuda.synchronize()
    if spy is not None:
        spy.extend(calls)
    return {k: p.grad.clone() for k, p in tr.policy_net.named_parameters() if p.grad is not None}, rec


def _close(g0, g1, floor):
    """every gradient within 1e-5 of max(floor, its scale): floor 1e-3 where only the order of fp32 sums differs (two chains
    against one, on the same record); floor 1 (the bar of test_trainer_gpu.py's record-against-recompute test at hid 128) where
    the recomputing backward forms inp and the gates again — inp = encoder + C(comm) through library products there, through the
    step launch's own matrix instructions in the record, which moves the last bits of every gate"""
    assert g0.keys() == g1.keys()
    for k in g0:
        err = float((g0[k] - g1[k]).abs().max())
        assert err <= 1e-5 * max(floor, float(g1[k].abs().max())), (k, err, float(g1[k].abs().max()))


def test_gate_record_at_hid_256_through_the_rollout():
    """The recorded rollout at hid 256: (h, c) of every slot the same bits with and without the gate record armed; the recorded
    gates reproduce the recorded next state; the inp rows (row stride H) reproduce the gates with the state that entered."""
    _, r1 = _update('pp_scaled', 6, 5, record=True)
    _, r0 = _update('pp_scaled', 6, 5, record=False)
    assert r1['gates'] and not r0['gates']
    assert torch.equal(r1['hs'], r0['hs']) and torch.equal(r1['cs'], r0['cs'])
    n = r1['n']
    g = r1['g'][:n - 1].double()
    assert tuple(r1['xh'].shape[1:]) == (6 * 32, H)
    c1 = g[..., H:2 * H] * r1['cs'][:n - 1].double() + g[..., :H] * g[..., 2 * H:3 * H]
    assert float((c1 - r1['cs'][1:n].double()).abs().max()) <= 1e-6
    assert float((g[..., 3 * H:] * torch.tanh(c1) - r1['hs'][1:n].double()).abs().max()) <= 2e-6
    fm = r1['knet'].f_module
    W = torch.cat([fm.weight_ih, fm.weight_hh], 1).detach().double()
    pre = torch.cat([r1['xh'][:n - 1].double(), r1['hs'][:n - 1].double()], 2) @ W.t() + (fm.bias_ih + fm.bias_hh).detach().double()
    assert float((torch.sigmoid(pre[..., :H]) - g[..., :H]).abs().max()) <= 1e-5
    assert float((torch.tanh(pre[..., 2 * H:3 * H]) - g[..., 2 * H:3 * H]).abs().max()) <= 1e-5


@pytest.mark.parametrize("wl,hid,collect", [("pp_scaled", 256, False), ("pp_scaled", 256, True), ("pp_scaled", 200, False),
                                            ("tj_hard", 256, True)])
def test_window_backward_at_hid_256_equals_the_recomputing_backward(wl, hid, collect):
    """The window path at hid 256 (and for hid 200 on its zero-padded twin at 256, gradients cut back by unpad_grads): asserted to
    run (ops.bptt_backward at H = 256), against the recomputing backward (args.record_gates=False) at 1e-5 (_close) — lock-step with detach points mid-window, and collection mode with episodes ending mid-window."""
    spy = []
    g1, r1 = _update(wl, 12, 8, record=True, collect=collect, spy=spy, hid_size=hid)
    assert r1['gates'] and spy and all(h == 256 for h in spy)
    spy0 = []
    g0, r0 = _update(wl, 12, 8, record=False, collect=collect, spy=spy0, hid_size=hid)
    assert not r0['gates'] and not spy0
    assert torch.equal(r1['hs'], r0['hs'])
    _close(g1, g0, 1.0)


def test_two_chains_at_hid_256_equal_one():
    """ic3_bptt.two_chains at hid 256 (E = 192: envs [0, 64) and [64, 192) on two streams) against the single chain."""
    from ic3net_amd import ops
    assert ops.first_chain_envs(192, 32) == 64
    g2, _ = _update('pp_scaled', 192, 4, two=True)
    g1, _ = _update('pp_scaled', 192, 4, two=False)
    _close(g2, g1, 1e-3)


def test_window_backward_at_hid_256_matches_autograd():
    """The native update at hid 256 on the one-launch rollout against loss.backward() through the autograd rollout replaying
    the same actions (trainer.py:128-225 both ways, detach points inside the episode)."""
    import bench
    from ic3net_amd import trainer as trmod
    E, T = 6, 7
    extra = dict(gamma=0.95, normalize_rewards=True, entr=0.01, value_coeff=0.01, advantages_per_action=False, batch_size=E * T,
                 detach_gap=3, max_steps=T)
    tr, a = bench.build_trainer('pp_scaled', E, 3, 70, 0)
    a.__dict__.update(extra)
    assert tr._native_update()
    tr._records = []
    batch, _ = tr.run_batch(0)
    assert tr._records[0].gates is not None
    tr.optimizer.zero_grad()
    tr.compute_grad_native(batch, tr._records)
    tr._records = None
    g1 = {k: p.grad.clone() for k, p in tr.policy_net.named_parameters() if p.grad is not None}
    tape = torch.stack(batch.action).clone()
    tr2, a2 = bench.build_trainer('pp_scaled', E, 3, 70, 0)
    a2.__dict__.update(extra)

    def taped(args, action_out, clock, out=None):
        out.copy_(tape[clock.t])
        return out
    orig = trmod.select_action
    trmod.select_action = taped
    try:
        a2.rollout_grad = True
        batch2, _ = tr2.run_batch(0)
        tr2.optimizer.zero_grad()
        tr2.compute_grad(batch2)
    finally:
        trmod.select_action = orig
    g2 = {k: p.grad for k, p in tr2.policy_net.named_parameters() if p.grad is not None}
    assert set(g1) == set(g2)
    for k in g1:
        scale = max(float(g2[k].abs().max()), 1e-6)
        np.testing.assert_allclose(g1[k].cpu().numpy() / scale, g2[k].cpu().numpy() / scale, rtol=0, atol=5e-4, err_msg=k)


def test_window_backward_at_the_benchmark_geometry():
    """One short window (T = 4) of config 5 at E = 8192 — 262 144 agent rows: the persistent grid of the communication backward,
    the two chains and the row tiles at the benchmarked shape — against the recomputing backward."""
    spy = []
    g1, r1 = _update('pp_scaled', 8192, 4, spy=spy)
    assert r1['gates'] and spy == [256]
    g0, r0 = _update('pp_scaled', 8192, 4, record=False)
    assert not r0['gates']
    _close(g1, g0, 1.0)
