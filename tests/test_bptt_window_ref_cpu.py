"""CPU: the float64 reference of the LSTM window backward (tests/bptt_window_ref.py) against torch float64 autograd through a
consistent forward of the policy's recurrent step (encoder + communication + LSTMCell + heads, one pass) — the lock-step form
(the state handed on detached every detach_gap steps) and the collection form (per-row cuts)."""
import numpy as np
import pytest
import torch

import bptt_window_ref as ref


def _tmix(x, alive, gate, avg):
    E, N, _ = x.shape
    al = torch.ones(E, N, dtype=torch.float64) if alive is None else torch.as_tensor(alive, dtype=torch.float64)
    g = al * (1.0 if gate is None else torch.as_tensor(gate, dtype=torch.float64))
    S = (g[:, :, None] * x).sum(1, keepdim=True)
    n_alive = al.sum(1)
    scale = torch.where(n_alive > 1, 1.0 / (n_alive - 1).clamp(min=1), torch.ones_like(n_alive)) if avg else torch.ones_like(n_alive)
    return g[:, :, None] * (S - g[:, :, None] * x) * scale[:, None, None]


CASES = [dict(T=5, gap=2), dict(T=4, gap=2), dict(T=5, gap=3, avg=False), dict(T=5, gap=0, comm_zero=True), dict(T=6, gap=4),
         dict(T=1, gap=1), dict(T=3, gap=0, masks=False)]


@pytest.mark.parametrize("collect", [False, True], ids=["lockstep", "collection"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
def test_reference_equals_float64_autograd(case, collect):
    """Every output of window_backward within 1e-10 of autograd: dgates = dL/d(gate pre-activations), d inp, dL/d(h, c) entering the
    window, the gradients of C, the LSTM's weights and bias (the tile rows summed) and of the encoder.  Lock-step: (h, c) detached
    behind every step t with (t + 1) % gap == 0 — T = 4, gap = 2 detaches the window's last step, whose arriving dh / dc then count
    for nothing.  Collection: h = keep h1 + (1 - keep) h1.detach(), c likewise, the entering state times row_live; a fresh env has
    alive = 1, gate = 0, and row_keep of the slot before is 0; dh arrives at the last slot as is, dc times row_keep[T - 1]."""
    T, gap = case['T'], case['gap']
    avg, comm_zero, masks = case.get('avg', True), case.get('comm_zero', False), case.get('masks', True)
    if collect:
        gap = 0                                                  # (lock-step carries no row factors, collection no detach_gap)
    E, N, H, OT, D = 5, 3, 8, 4, 7
    R = E * N
    rng = np.random.default_rng(100 * T + gap + 7 * collect)
    td = lambda a: torch.tensor(a, dtype=torch.float64)
    w_ih, w_hh = rng.standard_normal((4 * H, H)) / H ** 0.5, rng.standard_normal((4 * H, H)) / H ** 0.5
    bias, cw = rng.standard_normal(4 * H) * 0.1, rng.standard_normal((H, H)) / H ** 0.5
    wt, w_heads = rng.standard_normal((D, H)) * 0.3, rng.standard_normal((OT, H)) / H ** 0.5
    obs = rng.standard_normal((T, R, D))
    dhead = rng.standard_normal((T, R, OT))
    dh_T, dc_T = rng.standard_normal((R, H)), rng.standard_normal((R, H))
    alive = [None] + [(rng.random((E, N)) < 0.8).astype(np.int32) for _ in range(T - 1)] if masks else None
    gate = [(rng.random((E, N)) < 0.6).astype(np.int32) for _ in range(T)] if masks else None
    live = keep = None
    if collect:
        live, keep, fresh = ref.collection_cuts(rng, T, E, N)
        if masks:
            for t in range(T):
                gate[t][fresh[t]] = 0
                if alive[t] is not None:
                    alive[t][fresh[t]] = 1
        else:                                                    # (no masks: nobody may be fresh — M_t would mix a dropped state in)
            live[:], keep[:-1] = 1.0, (rng.random((T - 1, R)) < 0.7)
    P = {k: td(v).requires_grad_(True) for k, v in dict(w_ih=w_ih, w_hh=w_hh, bias=bias, cw=cw, wt=wt).items()}
    h0 = td(rng.standard_normal((R, H)) * 0.5).requires_grad_(True)
    c0 = td(rng.standard_normal((R, H)) * 0.5).requires_grad_(True)
    h, c = h0, c0
    rec = dict(gates=[], hs=[], cs=[], inp=[], pre=[])
    loss = 0.0
    for t in range(T):
        rec['hs'].append(h.detach().numpy().copy())
        rec['cs'].append(c.detach().numpy().copy())
        lv = td(live[t]).reshape(R, 1) if collect else 1.0
        h_in, c_in = h * lv, c * lv
        x = td(obs[t]) @ P['wt']
        if comm_zero:
            inp = x + 0.0
        else:
            comm = _tmix(h_in.reshape(E, N, H), None if alive is None else alive[t], None if gate is None else gate[t], avg)
            inp = x + comm.reshape(R, H) @ P['cw'].t()
        inp.retain_grad()
        pre = inp @ P['w_ih'].t() + h_in @ P['w_hh'].t() + P['bias']
        pre.retain_grad()
        i, f, g, o = pre[:, :H].sigmoid(), pre[:, H:2 * H].sigmoid(), pre[:, 2 * H:3 * H].tanh(), pre[:, 3 * H:].sigmoid()
        c1 = f * c_in + i * g
        h1 = o * c1.tanh()
        loss = loss + ((h1 @ td(w_heads).t()) * td(dhead[t])).sum()
        rec['gates'].append(torch.cat([i, f, g, o], 1).detach().numpy())
        rec['inp'].append(inp)
        rec['pre'].append(pre)
        if collect:
            kp = td(keep[t]).reshape(R, 1)
            h = h1 if t == T - 1 else kp * h1 + (1 - kp) * h1.detach()          # (dh arrives at the last slot as is)
            c = kp * c1 + (1 - kp) * c1.detach()
        elif gap > 0 and (t + 1) % gap == 0:
            h, c = h1.detach(), c1.detach()
        else:
            h, c = h1, c1
    loss = loss + (h * td(dh_T)).sum() + (c * td(dc_T)).sum()
    loss.backward()
    got = ref.window_backward(np.stack(rec['gates']), np.stack(rec['hs']), np.stack(rec['cs']), dhead, w_heads, w_ih, w_hh, dh_T, dc_T,
                              E, N, c_weight=cw, alive=alive, gate=gate, row_live=live, row_keep=keep, detach_gap=gap, mode_avg=avg,
                              comm_zero=comm_zero, obs=obs, inp=np.stack([v.detach().numpy() for v in rec['inp']]))
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    worst = {}
    for t in range(T):
        worst['dgates'] = max(worst.get('dgates', 0), ref.rel_err(got['dgates'][t], zero(rec['pre'][t]).numpy()))
        worst['dinp'] = max(worst.get('dinp', 0), ref.rel_err(got['dxh'][t][:, :H], zero(rec['inp'][t]).numpy()))
    # (what leaves the window is dL/d(the state the first step's cell saw): the row_live[0] factor in front of it belongs to the
    #  slot before, whose row_keep the caller applies — autograd's leaf sits in front of that factor)
    lv0 = live[0].reshape(R, 1) if collect else 1.0
    worst['dh'] = ref.rel_err(got['dh'] * lv0, zero(h0).numpy())
    worst['dc'] = ref.rel_err(got['dc'] * lv0, zero(c0).numpy())
    worst['dbias'] = ref.rel_err(got['dbias_rows'].sum(0), zero(P['bias']).numpy())
    worst['dW'] = ref.rel_err(got['dW'], torch.cat([zero(P['w_ih']), zero(P['w_hh'])], 1).t().numpy())
    worst['enc_dwt'] = ref.rel_err(got['enc_dwt'], zero(P['wt']).numpy())
    if not comm_zero:
        worst['dcw'] = ref.rel_err(got['dcw'], zero(P['cw']).numpy())
    else:
        assert not got['dcw'].any()
    assert max(worst.values()) <= 1e-10, worst
    assert np.abs(got['dgates']).max() > 1e-3 and np.abs(got['dh']).max() > 1e-3      # (not a comparison of zeros)


def test_bias_rows_are_the_tile_sums():
    """dbias_rows: row w holds the column sums of rows [64 w, 64 w + 64) of every step's dgates (a ragged last tile included)."""
    rng = np.random.default_rng(2)
    T, E, N, H, OT = 2, 50, 3, 4, 2
    R = E * N
    got = ref.window_backward(ref.activated(rng.standard_normal((T, R, 4 * H))), rng.standard_normal((T, R, H)),
                              rng.standard_normal((T, R, H)), rng.standard_normal((T, R, OT)), rng.standard_normal((OT, H)),
                              rng.standard_normal((4 * H, H)), rng.standard_normal((4 * H, H)), rng.standard_normal((R, H)),
                              rng.standard_normal((R, H)), E, N, comm_zero=True)
    assert got['dbias_rows'].shape == (3, 4 * H)
    for w in range(3):
        np.testing.assert_allclose(got['dbias_rows'][w], got['dgates'][:, 64 * w:64 * w + 64].sum((0, 1)), rtol=1e-12, atol=1e-12)
