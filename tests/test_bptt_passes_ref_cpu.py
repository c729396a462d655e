"""CPU: the float64 reference of the comm_passes > 1 window (tests/bptt_passes_ref.py: forward and backward) against torch float64
autograd through P chained torch.nn.LSTMCell calls per step (comm.py:179-218: every pass mixes the hidden state the previous pass
left, through its own C_i or a shared one, and feeds the same f_module), at H = 8, N = 3, E = 4, T = 3."""
import numpy as np
import pytest
import torch

import bptt_passes_ref as ref
from test_bptt_window_ref_cpu import _tmix

CASES = {
    'P2-own-C': dict(P=2),
    'P3-shared-C': dict(P=3, share=True),
    'P2-sum-mode': dict(P=2, avg=False),
    'P2-comm-zero': dict(P=2, comm_zero=True),
    'P2-detach-gap2': dict(P=2, gap=2),                          # one detach point inside the window (behind step 1)
    'P3-detach-last-step': dict(P=3, gap=3),                     # the window's last step detached: the arriving dh / dc count for nothing
}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_float64_autograd(name):
    """The forward records (activated gates, inp, the state entering every pass) within 1e-12 of the torch forward, and every output of
    window_backward within 1e-10 of autograd: dL/d(gate pre-activations) and d inp of every (step, pass), dL/d(h, c) entering the
    window, the gradients of every C_i (weight and bias; shared: their sum), of the LSTM's weights and bias and of the encoder."""
    case = CASES[name]
    P, share, avg, comm_zero, gap = case['P'], case.get('share', False), case.get('avg', True), case.get('comm_zero', False), case.get('gap', 0)
    E, N, H, T, OT, D = 4, 3, 8, 3, 4, 7
    R = E * N
    rng = np.random.default_rng(sum(map(ord, name)))
    td = lambda a: torch.tensor(a, dtype=torch.float64)
    cell = torch.nn.LSTMCell(H, H).double()
    nC = 1 if share else P
    cmods = [torch.nn.Linear(H, H).double() for _ in range(nC)]
    enc = torch.nn.Linear(D, H).double()
    w_heads = rng.standard_normal((OT, H)) / H ** 0.5
    obs, dhead = rng.standard_normal((T, R, D)), rng.standard_normal((T, R, OT))
    dh_T, dc_T = rng.standard_normal((R, H)), rng.standard_normal((R, H))
    alive = [None] + [(rng.random((E, N)) < 0.8).astype(np.int32) for _ in range(T - 1)]
    gate = [(rng.random((E, N)) < 0.6).astype(np.int32) for _ in range(T)]
    h0 = td(rng.standard_normal((R, H)) * 0.5).requires_grad_(True)
    c0 = td(rng.standard_normal((R, H)) * 0.5).requires_grad_(True)
    h, c = h0, c0
    pres, inps = {}, {}
    loss = 0.0
    for t in range(T):
        x = enc(td(obs[t]))
        for i in range(P):
            C = cmods[0 if share else i]
            comm = torch.zeros(R, H, dtype=torch.float64) if comm_zero else _tmix(h.reshape(E, N, H), alive[t], gate[t], avg).reshape(R, H)
            inp = x + C(comm)
            inp.retain_grad()
            # torch.nn.LSTMCell's arithmetic with the pre-activations on the graph (checked against the module itself below)
            pre = inp @ cell.weight_ih.t() + h @ cell.weight_hh.t() + cell.bias_ih + cell.bias_hh
            pre.retain_grad()
            g_i, g_f, g_g, g_o = pre[:, :H].sigmoid(), pre[:, H:2 * H].sigmoid(), pre[:, 2 * H:3 * H].tanh(), pre[:, 3 * H:].sigmoid()
            c1 = g_f * c + g_i * g_g
            h1 = g_o * c1.tanh()
            with torch.no_grad():
                hm, cm = cell(inp, (h, c))
                assert torch.allclose(hm, h1, atol=1e-13, rtol=0) and torch.allclose(cm, c1, atol=1e-13, rtol=0)
            pres[i, t], inps[i, t] = pre, inp
            h, c = h1, c1
        loss = loss + ((h @ td(w_heads).t()) * td(dhead[t])).sum()
        if gap > 0 and (t + 1) % gap == 0:
            h, c = h.detach(), c.detach()
    loss = loss + (h * td(dh_T)).sum() + (c * td(dc_T)).sum()
    loss.backward()
    num = lambda v: v.detach().numpy()
    cws = [num(cmods[0 if share else i].weight) for i in range(P)]
    cbs = [num(cmods[0 if share else i].bias) for i in range(P)]
    w_ih, w_hh = num(cell.weight_ih), num(cell.weight_hh)
    fwd = ref.window_forward(num(enc(td(obs))), num(h0), num(c0), cws, cbs, w_ih, w_hh, num(cell.bias_ih + cell.bias_hh), E, N,
                             alive=alive, gate=gate, mode_avg=avg, comm_zero=comm_zero, detach_gap=gap)
    for i in range(P):
        for t in range(T):
            assert ref.rel_err(fwd['gates'][i, t], ref.activated(num(pres[i, t]))) <= 1e-12
            assert ref.rel_err(fwd['inp'][i, t], num(inps[i, t])) <= 1e-12
    got = ref.window_backward(fwd['gates'], fwd['hs'], fwd['cs'], dhead, w_heads, w_ih, w_hh, dh_T, dc_T, E, N, c_weights=cws,
                              alive=alive, gate=gate, detach_gap=gap, mode_avg=avg, comm_zero=comm_zero, obs=obs, inp=fwd['inp'])
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
    # the per-pass bias partials hold the C_i.bias gradient: (column sums of pass i's dgates) . W_ih = column sums of pass i's d inp
    for i in range(P):
        assert ref.rel_err(got['dbias_rows'][i].sum(0) @ w_ih, got['dcb'][i]) <= 1e-12
