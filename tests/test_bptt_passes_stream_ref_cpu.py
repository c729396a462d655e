"""CPU: the float64 reference of the comm_passes > 1 window in collection mode (tests/bptt_passes_stream_ref.py) against torch float64
autograd through P chained LSTM cells per slot, with the cuts written into the graph: the state leaving slot t is handed on as
keep * s + ((1 - keep) * s).detach() (the value passes, the gradient only where keep = 1), and an env that starts an episode at slot t
runs on s - (fresh * s).detach() (zeros in the forward, constants in the backward) with nobody dead and everyone gated off in every
pass of that step.  H = 8, N = 3, E = 5, T = 4."""
import numpy as np
import pytest
import torch

import bptt_passes_stream_ref as ref
from test_bptt_window_ref_cpu import _tmix

E, N, H, T, OT, D = 5, 3, 8, 4, 4, 7
R = E * N

CASES = {
    # env 0 starts at slot 0, env 2 mid-window, keep = 0 in front of each start, one detach-style zero elsewhere
    'P2-product': dict(P=2, cuts=lambda: ref.product_cuts(T, E, [(0, 0), (2, 2)], [(1, 4)])),
    'P3-shared-product-last-slot-cut': dict(P=3, share=True, cuts=lambda: ref.product_cuts(T, E, [(1, 1), (3, 3)], [(3, 0), (0, 2)])),
    'P2-independent': dict(P=2, cuts=lambda: ref.independent_cuts(7, T, E)),
    'P2-independent-sum-mode': dict(P=2, avg=False, cuts=lambda: ref.independent_cuts(8, T, E)),
    'P2-independent-comm-zero': dict(P=2, comm_zero=True, cuts=lambda: ref.independent_cuts(9, T, E)),
    'P2-independent-no-gate': dict(P=2, no_gate=True, cuts=lambda: ref.independent_cuts(10, T, E)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_stream_reference_equals_float64_autograd(name):
    """Forward records within 1e-12 of the torch forward and every output of stream_backward within 1e-10 of autograd: dL/d(gate
    pre-activations) and d inp of every (slot, pass), dL/d(h, c) entering the window, every parameter's gradient.  The same window
    as two chunks (slots [2, 4) then [0, 2), the second fed what the first returned) gives the whole window's numbers."""
    case = CASES[name]
    P, share, avg, comm_zero = case['P'], case.get('share', False), case.get('avg', True), case.get('comm_zero', False)
    fresh, keep = case['cuts']()
    assert fresh.any() and (~keep).any() and keep.any()
    rng = np.random.default_rng(sum(map(ord, name)))
    td = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    cell = torch.nn.LSTMCell(H, H).double()
    cmods = [torch.nn.Linear(H, H).double() for _ in range(1 if share else P)]
    enc = torch.nn.Linear(D, H).double()
    w_heads = rng.standard_normal((OT, H)) / H ** 0.5
    obs, dhead = rng.standard_normal((T, R, D)), rng.standard_normal((T, R, OT))
    dh_T, dc_T = rng.standard_normal((R, H)), rng.standard_normal((R, H))
    alive = [None] + [(rng.random((E, N)) < 0.8).astype(np.int32) for _ in range(T - 1)]
    gate = None if case.get('no_gate') else [(rng.random((E, N)) < 0.6).astype(np.int32) for _ in range(T)]
    fr_rows, kp_rows = td(ref.rows(fresh, N)), td(ref.rows(keep, N))
    h0 = td(rng.standard_normal((R, H)) * 0.5).requires_grad_(True)
    c0 = td(rng.standard_normal((R, H)) * 0.5).requires_grad_(True)
    h, c = h0, c0
    pres, inps, hs_rec, cs_rec = {}, {}, [], []
    loss = 0.0
    ones = np.ones((E, N), np.int32)
    for t in range(T):
        hs_rec.append(h.detach().numpy().copy())                 # what a record holds: the state as the slot before left it
        cs_rec.append(c.detach().numpy().copy())
        h, c = h - (fr_rows[t] * h).detach(), c - (fr_rows[t] * c).detach()
        fr = fresh[t][:, None]
        al = None if alive[t] is None else np.where(fr, 1, alive[t]).astype(np.int32)
        gt = None if gate is None else np.where(fr, 0, gate[t]).astype(np.int32)
        x = enc(td(obs[t]))
        for i in range(P):
            C = cmods[0 if share else i]
            comm = torch.zeros(R, H, dtype=torch.float64) if comm_zero else _tmix(h.reshape(E, N, H), al, gt, avg).reshape(R, H)
            inp = x + C(comm)
            inp.retain_grad()
            pre = inp @ cell.weight_ih.t() + h @ cell.weight_hh.t() + cell.bias_ih + cell.bias_hh
            pre.retain_grad()
            g_i, g_f, g_g, g_o = pre[:, :H].sigmoid(), pre[:, H:2 * H].sigmoid(), pre[:, 2 * H:3 * H].tanh(), pre[:, 3 * H:].sigmoid()
            c1 = g_f * c + g_i * g_g
            h1 = g_o * c1.tanh()
            pres[i, t], inps[i, t] = pre, inp
            h, c = h1, c1
        loss = loss + ((h @ td(w_heads).t()) * td(dhead[t])).sum()
        h = kp_rows[t] * h + ((1 - kp_rows[t]) * h).detach()
        c = kp_rows[t] * c + ((1 - kp_rows[t]) * c).detach()
    loss = loss + (h * td(dh_T)).sum() + (c * td(dc_T)).sum()
    loss.backward()
    num = lambda v: v.detach().numpy()
    cws = [num(cmods[0 if share else i].weight) for i in range(P)]
    cbs = [num(cmods[0 if share else i].bias) for i in range(P)]
    w_ih, w_hh = num(cell.weight_ih), num(cell.weight_hh)
    hs_rec, cs_rec = np.stack(hs_rec), np.stack(cs_rec)
    fwd = ref.stream_forward(num(enc(td(obs))), hs_rec, cs_rec, fresh, cws, cbs, w_ih, w_hh, num(cell.bias_ih + cell.bias_hh), E, N,
                             alive=alive, gate=gate, mode_avg=avg, comm_zero=comm_zero)
    for i in range(P):
        for t in range(T):
            assert ref.rel_err(fwd['gates'][i, t], ref.activated(num(pres[i, t]))) <= 1e-12
            assert ref.rel_err(fwd['inp'][i, t], num(inps[i, t])) <= 1e-12

    def backward(t0, t1, dh, dc):
        return ref.stream_backward(fwd['gates'][:, t0:t1], fwd['hs'][:, t0:t1], fwd['cs'][:, t0:t1], hs_rec[t0:t1], cs_rec[t0:t1],
                                   fresh[t0:t1], keep[t0:t1], dhead[t0:t1], w_heads, w_ih, w_hh, dh, dc, E, N, c_weights=cws,
                                   alive=alive[t0:t1], gate=None if gate is None else gate[t0:t1], mode_avg=avg, comm_zero=comm_zero,
                                   obs=obs[t0:t1], inp=fwd['inp'][:, t0:t1])
    got = backward(0, T, dh_T, dc_T)
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    worst = dict(dgates=0.0, dinp=0.0)
    for i in range(P):
        for t in range(T):
            worst['dgates'] = max(worst['dgates'], ref.rel_err(got['dgates'][i, t], zero(pres[i, t]).numpy()))
            worst['dinp'] = max(worst['dinp'], ref.rel_err(got['dxh'][i, t][:, :H], zero(inps[i, t]).numpy()))
    worst['dh'] = ref.rel_err(got['dh'], zero(h0).numpy())
    worst['dc'] = ref.rel_err(got['dc'], zero(c0).numpy())
    worst['dbias'] = ref.rel_err(got['dbias_rows'].sum((0, 1)), zero(cell.bias_ih).numpy())
    worst['dW'] = ref.rel_err(got['dW'], torch.cat([zero(cell.weight_ih), zero(cell.weight_hh)], 1).t().numpy())
    worst['enc_dwt'] = ref.rel_err(got['enc_dwt'], zero(enc.weight).t().numpy())
    worst['enc_db'] = ref.rel_err(got['enc_db'], zero(enc.bias).numpy())
    if share:
        worst['dcb'] = ref.rel_err(got['dcb'].sum(0), zero(cmods[0].bias).numpy())
        worst['dcw'] = ref.rel_err(got['dcw'].sum(0), zero(cmods[0].weight).numpy())
    else:
        for i in range(P):
            worst['dcb%d' % i] = ref.rel_err(got['dcb'][i], zero(cmods[i].bias).numpy())
            worst['dcw%d' % i] = ref.rel_err(got['dcw'][i], zero(cmods[i].weight).numpy())
    if comm_zero:
        assert not got['dcw'].any()
    assert max(worst.values()) <= 1e-10, worst
    assert np.abs(got['dgates']).max() > 1e-3 and np.abs(got['dh']).max() > 1e-3      # (not a comparison of zeros)
    # two chunks chained: the later one first, what it returns goes into the earlier one as it is
    late = backward(2, T, dh_T, dc_T)
    early = backward(0, 2, late['dh'], late['dc'])
    assert ref.rel_err(early['dh'], got['dh']) <= 1e-12 and ref.rel_err(early['dc'], got['dc']) <= 1e-12
    assert ref.rel_err(np.concatenate([early['dgates'], late['dgates']], 1), got['dgates']) <= 1e-12
    for k in ('dW', 'dcw', 'dcb', 'enc_dwt', 'enc_db', 'dbias_rows'):
        assert ref.rel_err(early[k] + late[k], got[k]) <= 1e-12, k


def test_the_cut_helpers():
    fresh, keep = ref.product_cuts(4, 3, [(0, 0), (2, 1)], [(3, 2)])
    assert fresh.sum() == 2 and fresh[0, 0] and fresh[2, 1]
    assert (~keep).sum() == 2 and not keep[1, 1] and not keep[3, 2]
    al, gt = ref.cut_masks([None] * 4, [np.ones((3, 2), np.int32)] * 4, fresh, 2)
    assert all(a.all() for a in al) and not gt[0][0].any() and gt[0][1:].all() and not gt[2][1].any() and gt[1].all()
    assert ref.cut_masks(None, None, fresh, 2) == (None, None)
    h, c = ref.entering(np.ones((4, 6, 2)), np.ones((4, 6, 2)), fresh, 2)
    assert not h[0, :2].any() and h[0, 2:].all() and not c[2, 2:4].any() and h[1].all()
