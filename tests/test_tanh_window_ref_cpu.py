"""CPU: the float64 references of the two tanh window backwards (tests/tanh_window_ref.py) against torch float64 autograd through a
consistent forward — the tanh recurrence h_t = tanh(affine1(obs_t) + affine2(h_{t-1})) in its lock-step form (the state handed on
detached every detach_gap steps) and its collection form (per-row cuts, written as .detach() and multiplications in the forward),
and models.MLP's forward."""
import numpy as np
import pytest
import torch

import tanh_window_ref as ref

CASES = [dict(T=5, gap=2), dict(T=4, gap=2), dict(T=5, gap=3), dict(T=5, gap=0), dict(T=6, gap=4), dict(T=1, gap=1), dict(T=1, gap=0),
         dict(T=3, gap=1)]


@pytest.mark.parametrize("h_last", ['slot', 'separate'])
@pytest.mark.parametrize("collect", [False, True], ids=["lockstep", "collection"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
def test_rnn_reference_equals_float64_autograd(case, collect, h_last):
    """Every output of rnn_window_backward within 1e-12 of autograd: dz = dL/d(the steps' pre-activations), dL/dh entering the
    window, the gradients of affine2's weight and bias (the tile rows summed, and the column sum) and of the encoder.  Lock-step: h
    detached behind every step t with (t + 1) % gap == 0 — T = 4, gap = 2 detaches the window's last step, whose arriving dh then
    counts for nothing.  Collection: h = keep h_t + (1 - keep) h_t.detach() behind every step but the last (dh arrives at the last
    slot as is), the entering state times row_live; row_keep of the slot before a fresh one is 0.  h_last 'separate': the record
    has T slots and the last step's h_t comes in a buffer of its own."""
    T, gap = case['T'], case['gap']
    if collect:
        gap = 0                                                  # (lock-step carries no row factors, collection no detach_gap)
    E, N, H, OT, D = 27, 3, 8, 4, 7                              # R = 81: two tiles, the second ragged
    R = E * N
    rng = np.random.default_rng(100 * T + gap + 7 * collect)
    td = lambda a: torch.tensor(a, dtype=torch.float64)
    a2, b2 = rng.standard_normal((H, H)) / H ** 0.5, rng.standard_normal(H) * 0.1
    wt, b1, w_heads = rng.standard_normal((D, H)) * 0.3, rng.standard_normal(H) * 0.1, rng.standard_normal((OT, H)) / H ** 0.5
    obs, dhead, dh_T = rng.standard_normal((T, R, D)), rng.standard_normal((T, R, OT)), rng.standard_normal((R, H))
    live = keep = None
    if collect:
        live, keep, _ = ref.collection_cuts(rng, T, E, N)
    P = {k: td(v).requires_grad_(True) for k, v in dict(a2=a2, b2=b2, wt=wt, b1=b1).items()}
    h0 = td(rng.standard_normal((R, H)) * 0.5).requires_grad_(True)
    h = h0
    hs, pre = [], []
    loss = 0.0
    for t in range(T):
        hs.append(h.detach().numpy().copy())
        h_in = h * td(live[t]).reshape(R, 1) if collect else h
        z = td(obs[t]) @ P['wt'] + P['b1'] + h_in @ P['a2'].t() + P['b2']
        z.retain_grad()
        pre.append(z)
        h1 = torch.tanh(z)
        loss = loss + ((h1 @ td(w_heads).t()) * td(dhead[t])).sum()
        if collect:
            kp = td(keep[t]).reshape(R, 1)
            h = h1 if t == T - 1 else kp * h1 + (1 - kp) * h1.detach()
        elif gap > 0 and (t + 1) % gap == 0:
            h = h1.detach()
        else:
            h = h1
    loss = loss + (h * td(dh_T)).sum()
    loss.backward()
    last = h1.detach().numpy().copy()
    if h_last == 'slot':
        rec, sep = np.stack(hs + [last]), None
    else:
        rec, sep = np.stack(hs), last
    got = ref.rnn_window_backward(rec, sep, dhead, w_heads, a2, dh_T, row_live=live, row_keep=keep, detach_gap=gap, obs=obs)
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    worst = dict(dz=max(ref.rel_err(got['dz'][t], zero(pre[t]).numpy()) for t in range(T)))
    # (what leaves the window is dL/d(the state the first step saw): the row_live[0] factor in front of it belongs to the slot
    #  before, whose row_keep the caller applies — autograd's leaf sits in front of that factor)
    worst['dh'] = ref.rel_err(got['dh'] * (live[0].reshape(R, 1) if collect else 1.0), zero(h0).numpy())
    worst['a2_grad'] = ref.rel_err(got['a2_grad'], zero(P['a2']).numpy())
    worst['dbias_cols'] = ref.rel_err(got['dbias_cols'], zero(P['b2']).numpy())
    worst['dbias_tiles'] = ref.rel_err(got['dbias_tiles'].sum(0), zero(P['b2']).numpy())
    worst['enc_dwt'] = ref.rel_err(got['enc_dwt'], zero(P['wt']).numpy())
    worst['enc_db'] = ref.rel_err(got['enc_db'], zero(P['b1']).numpy())
    assert max(worst.values()) <= 1e-12, worst
    assert got['dbias_tiles'].shape == (2, H)
    np.testing.assert_allclose(got['dbias_tiles'][1], got['dz'][:, 64:].sum((0, 1)), rtol=1e-12, atol=1e-12)
    assert np.abs(got['dz']).max() > 1e-3 and np.abs(got['dh']).max() > 1e-3            # (not a comparison of zeros)


def test_a_detached_last_step_ignores_the_arriving_dh():
    """T a multiple of detach_gap: the dh handed in reaches nothing — every output the same for two different ones."""
    w = ref.make_rnn_window(3, 4, 5, 3, 8, 4)
    a = ref.rnn_reference_of(w, detach_gap=2)
    w['dh'] = w['dh'] + 1.0
    b = ref.rnn_reference_of(w, detach_gap=2)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    c = ref.rnn_reference_of(w, detach_gap=3)
    assert np.abs(c['dz'][3] - a['dz'][3]).max() > 1e-3


def test_the_record_makers():
    """make_rnn_window: T + 1 slots or T slots and a separate h_last, float32 and contiguous, cuts only in collection mode (and as
    collection_cuts couples them: nothing crosses into a fresh slot)."""
    w = ref.make_rnn_window(1, 3, 4, 5, 8, 6)
    assert w['hs'].shape == (4, 20, 8) and w['h_last'] is None and w['row_live'] is None and w['row_keep'] is None
    w = ref.make_rnn_window(1, 3, 40, 5, 8, 6, collect=True, h_last='separate')
    assert w['hs'].shape == (3, 200, 8) and w['h_last'].shape == (200, 8)
    assert w['row_live'].shape == (3, 200) and w['row_keep'].shape == (3, 200)
    assert not (w['row_keep'][:-1] * (1 - w['row_live'][1:])).any() and (w['row_live'] == 0).any() and (w['row_keep'] == 0).any()
    for v in w.values():
        assert not isinstance(v, np.ndarray) or (v.dtype == np.float32 and v.flags.c_contiguous)
    m = ref.make_mlp_window(1, 3, 4, 5, 8, 6, 11)
    assert m['h'].shape == (3, 20, 8) and m['enc_wt'].shape == (11, 8) and np.abs(m['h']).max() < 1


@pytest.mark.parametrize("T,E", [(1, 5), (3, 27)])
def test_mlp_reference_equals_float64_autograd(T, E):
    """Every output of mlp_window_backward within 1e-12 of autograd through models.MLP's forward (models.py:23-34): x1, dz =
    dL/d(affine2's pre-activation), de = dL/d(affine1's), the gradients of affine2 (weight; bias as column sum and as tile rows over
    the window's T x R rows) and of the encoder."""
    N, H, OT, D = 3, 8, 4, 7
    R = E * N
    rng = np.random.default_rng(T)
    td = lambda a: torch.tensor(a, dtype=torch.float64)
    a2, b2 = rng.standard_normal((H, H)) / H ** 0.5, rng.standard_normal(H) * 0.1
    wt, b1, w_heads = rng.standard_normal((D, H)) * 0.3, rng.standard_normal(H) * 0.1, rng.standard_normal((OT, H)) / H ** 0.5
    obs, dhead = rng.standard_normal((T, R, D)), rng.standard_normal((T, R, OT))
    P = {k: td(v).requires_grad_(True) for k, v in dict(a2=a2, b2=b2, wt=wt, b1=b1).items()}
    e = td(obs) @ P['wt'] + P['b1']
    e.retain_grad()
    x1 = torch.tanh(e)
    z = x1 @ P['a2'].t() + P['b2'] + x1
    z.retain_grad()
    h = torch.tanh(z)
    ((h @ td(w_heads).t()) * td(dhead)).sum().backward()
    got = ref.mlp_window_backward(obs, wt, b1, h.detach().numpy(), dhead, w_heads, a2)
    worst = dict(x1=ref.rel_err(got['x1'], x1.detach().numpy()), dz=ref.rel_err(got['dz'], z.grad.numpy()),
                 de=ref.rel_err(got['de'], e.grad.numpy()), a2_grad=ref.rel_err(got['a2_grad'], P['a2'].grad.numpy()),
                 dbias_cols=ref.rel_err(got['dbias_cols'], P['b2'].grad.numpy()),
                 dbias_tiles=ref.rel_err(got['dbias_tiles'].sum(0), P['b2'].grad.numpy()),
                 enc_dwt=ref.rel_err(got['enc_dwt'], P['wt'].grad.numpy()), enc_db=ref.rel_err(got['enc_db'], P['b1'].grad.numpy()))
    assert max(worst.values()) <= 1e-12, worst
    assert got['dbias_tiles'].shape == ((T * R + 63) // 64, H)
    assert np.abs(got['dz']).max() > 1e-3 and np.abs(got['de']).max() > 1e-3
