"""GPU: the LSTM cell's weight gradient of a window at hid 256 on the HIP kernels (ic3_lstm_weight_grad_wide through
ops.lstm_weight_grad) — against float64 in both arithmetics, and through whole updates of config 5's grid (and a padded hid 200)
against the two library products it replaces (bptt._weight_grad_products behind args.lstm_wgrad_kernel=False)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 256


@pytest.mark.parametrize("split", [True, False], ids=["bf16x9", "fp32"])
@pytest.mark.parametrize("T,R,live", [(1, 17, False), (3, 1000, True), (7, 333, True), (2, 30000, False)])
def test_weight_gradient_at_hid_256_against_float64(T, R, live, split):
    """ops.lstm_weight_grad at H = 256 over T x R rows against the float64 product of [inp | h * live]^T . dgates, added on top of
    ones; twice, the same bits.  One ragged stage (17 rows); slices that end off a 16-row boundary, with the mask (3000 and 2331
    rows); 60 000 rows: several stages in every slice of the one round.  inp at row stride H (the record's layout at 256), in the
    (3, 1000) case also as the first half of rows of 2H.  The bar is the one of the test at 64 / 128 for the same unit-normal
    operands (test_gates_backward_gpu.py): 2e-6 . sqrt(T R) . 16."""
    from ic3net_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(H + T + R)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    xh, hs, dg = rn(T, R, 2 * H), rn(T, R, H), rn(T, R, 4 * H)
    lv = (torch.rand((T, R), device='cuda', generator=gen) < 0.8).float() if live else None
    x = torch.cat([xh[:, :, :H].double(), hs.double() * (lv.double().unsqueeze(2) if live else 1.0)], 2).view(T * R, 2 * H)
    want = 1.0 + x.t() @ dg.double().view(T * R, 4 * H)
    tol = 2e-6 * (T * R) ** 0.5 * 16
    before = dg.clone()
    inps = [xh[:, :, :H].contiguous()] + ([xh] if (T, R) == (3, 1000) else [])
    for inp in inps:
        outs = []
        for _ in range(2):
            dW = torch.ones((2 * H, 4 * H), device='cuda')
            ops.lstm_weight_grad(inp, hs, dg, dW, row_live=lv, split=split)
            outs.append(dW)
        err = float((outs[0].double() - want).abs().max())
        print("T %d R %d ldi %d split %s: max err %.3g (bar %.3g)" % (T, R, inp.shape[-1], split, err, tol))
        assert err <= tol
        assert torch.equal(outs[0], outs[1])
    assert torch.equal(dg, before)


def _update(E, T, collect, kernel, **over):
    """One recorded batch of pp_scaled through Trainer.run_batch + compute_grad_native (detach_gap 3), with spies on the window
    backward and on both weight-gradient paths.  Returns (grads, the recorded h of every window, what the spies saw)."""
    import bench
    from ic3net_amd import bptt, ops
    tr, a = bench.build_trainer('pp_scaled', E, 3, 0, 0, **over)
    a.max_steps, a.batch_size = T, E * T * (2 if collect else 1)
    a.detach_gap = 3
    a.entr, a.value_coeff, a.gamma, a.normalize_rewards, a.advantages_per_action = 0.01, 0.01, 0.9, False, False
    a.record_gates, a.auto_reset, a.bptt_two_chains = True, collect, True
    if not kernel:
        a.lstm_wgrad_kernel = False
    assert tr._native_update()
    tr._records = []
    batch, _ = tr.run_batch(0)
    recs = tr._records
    hs = torch.cat([r.hs[:r.n] for r in recs]).clone()
    seen = dict(windows=0, kernel_H=[], products=0, record_kept=[])
    left = []                                                    # dgates as ops.bptt_backward left them in the record
    orig_b, orig_k, orig_p = ops.bptt_backward, ops.lstm_weight_grad, bptt._weight_grad_products

    def window(*args, **kw):
        out = orig_b(*args, **kw)
        seen['windows'] += 1
        left.append(args[5][:args[1]].clone())                   # (gates[:T])
        return out

    def by_kernel(inp, h_prev, dgates, dW, **kw):
        out = orig_k(inp, h_prev, dgates, dW, **kw)
        seen['kernel_H'].append(h_prev.shape[-1])
        seen['record_kept'].append(torch.equal(dgates, left[-1]))
        return out

    def by_products(rec, T_, R_, H_, dW, row_live):
        out = orig_p(rec, T_, R_, H_, dW, row_live)
        seen['products'] += 1
        seen['record_kept'].append(torch.equal(rec.gates[:T_], left[-1]))
        return out
    ops.bptt_backward, ops.lstm_weight_grad, bptt._weight_grad_products = window, by_kernel, by_products
    try:
        tr.optimizer.zero_grad()
        tr.compute_grad_native(batch, recs)
    finally:
        ops.bptt_backward, ops.lstm_weight_grad, bptt._weight_grad_products = orig_b, orig_k, orig_p
        tr._records = None
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in tr.policy_net.named_parameters() if p.grad is not None}, hs, seen


@pytest.mark.parametrize("hid,collect", [(256, False), (256, True), (200, False)], ids=["h256", "h256-collect", "h200-padded"])
def test_update_at_hid_256_runs_the_kernel_and_equals_the_library_products(hid, collect):
    """The update of config 5's grid (12 envs of 32 agents, T = 8): ops.lstm_weight_grad once per window at H = 256 (hid 200: on its
    zero-padded twin) and no call of bptt._weight_grad_products; with args.lstm_wgrad_kernel=False the other way round.  The same
    rollout (recorded h the same bits), every gradient within 1e-5 . max(1, max|g|) of the library path's — the bar
    test_bptt_h256_gpu.py puts on two hid-256 backwards of one record.  Collection mode: the kernel leaves the record's dgates as
    the window backward wrote them; the library path scaled them by row_live in place."""
    g1, hs1, s1 = _update(12, 8, collect, True, hid_size=hid)
    assert s1['windows'] >= 1 and s1['kernel_H'] == [256] * s1['windows'] and s1['products'] == 0
    g0, hs0, s0 = _update(12, 8, collect, False, hid_size=hid)
    assert s0['windows'] == s1['windows'] and s0['products'] == s0['windows'] and not s0['kernel_H']
    assert torch.equal(hs1, hs0)
    assert g1.keys() == g0.keys()
    for k in g1:
        err, scale = float((g1[k] - g0[k]).abs().max()), float(g0[k].abs().max())
        print("%-28s max err %.3g, max |g| %.3g" % (k, err, scale))
    for k in g1:
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-5 * max(1.0, float(g0[k].abs().max())), k
    assert all(s1['record_kept'])
    if collect:
        assert not any(s0['record_kept'])
