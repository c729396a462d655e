"""TEST INFRASTRUCTURE: the float64 references of the two tanh window backwards — ic3_rnn_backward (IRIC / IC with the tanh recurrence)
and ic3_mlp_backward (models.MLP), include/ic3_rollout.h — closed-form backwards over the recorded steps, numpy only, shared by the
host-build and the GPU tests of the two calls (and themselves checked against torch float64 autograd through a consistent forward:
tests/test_tanh_window_ref_cpu.py).  The sibling of bptt_window_ref.py (the LSTM window).  Nothing under ic3net_amd/ imports this.

ic3_rnn_backward — h_t = tanh(affine1(obs_t) + affine2(h_{t-1})), heads and value on h_t; hs[t] = h_{t-1} the state that entered
step t, h_t = hs[t + 1] (the last step's: h_last when given).  Per step t = T-1 .. 0:
    det  = detach_gap > 0 and (t + 1) % detach_gap == 0
    dh_t = (0 if det else dh) + dhead[t] @ w_heads
    dz[t] = dh_t (1 - h_t^2)                                    (the gradient of step t's pre-activation)
    dh = (dz[t] @ A2) * row_keep[t - 1]                         (t = 0: no factor;  A2 = affine2.weight, (out, in))
    dA2 += dz[t]^T @ (row_live[t] hs[t]);  bias (both affines) += column sums of dz[t];  encoder: dWt += obs_t^T @ dz[t]

ic3_mlp_backward — e = affine1(obs), x1 = tanh(e), h = tanh(affine2(x1) + x1), heads and value on h; no state crosses a step:
    dz = (dhead @ w_heads)(1 - h^2);  de = (dz @ A2 + dz)(1 - x1^2);  dA2 = dz^T @ x1;  affine2.bias: column sums of dz
    encoder: dWt = sum_t obs_t^T @ de[t], db = column sums of de"""
import numpy as np

from bptt_window_ref import TILE, collection_cuts, rel_err  # noqa: F401  (re-exported: the tests take them from here)


def _f64(a):
    return np.asarray(a, np.float64)


def _tile_sums(rows):
    """(Q, H) -> (ceil(Q / 64), H): the column sums of every 64-row tile (a ragged last one included)"""
    return np.stack([rows[TILE * w:TILE * w + TILE].sum(0) for w in range((rows.shape[0] + TILE - 1) // TILE)])


def rnn_window_backward(hs, h_last, dhead, w_heads, a2, dh, row_live=None, row_keep=None, detach_gap=0, obs=None):
    """hs (>= T (+ 1), R, H), h_last None or (R, H), dhead (T, R, OT), w_heads (OT, H), a2 (H, H), dh (R, H) arriving at the last
    step, row_live / row_keep (T, R) or None, obs: None or T dense observations (R, obs_dim).  Everything is taken to float64.
    Returns a dict: dz (T, R, H), dh (R, H) leaving the first step, dbias_cols (H,), dbias_tiles (ceil(R / 64), H) — tile w's
    column sums over all steps —, a2_grad (H, H), and with obs: enc_dwt (obs_dim, H), enc_db (H,)."""
    hs, dhead, w_heads, a2 = _f64(hs), _f64(dhead), _f64(w_heads), _f64(a2)
    T, R, _ = dhead.shape
    H = hs.shape[-1]
    assert hs.shape[0] >= T + (h_last is None)
    dh = _f64(dh).copy()
    out = dict(dz=np.zeros((T, R, H)), dbias_tiles=np.zeros(((R + TILE - 1) // TILE, H)), a2_grad=np.zeros((H, H)))
    if obs is not None:
        out['enc_dwt'] = np.zeros((_f64(obs[0]).shape[-1], H))
    for t in range(T - 1, -1, -1):
        h_t = _f64(h_last) if (t == T - 1 and h_last is not None) else hs[t + 1]
        det = detach_gap > 0 and (t + 1) % detach_gap == 0
        dz = ((0.0 if det else dh) + dhead[t] @ w_heads) * (1.0 - h_t * h_t)
        out['dz'][t] = dz
        dh = dz @ a2
        if row_keep is not None and t > 0:
            dh = dh * _f64(row_keep[t - 1]).reshape(R, 1)
        live = 1.0 if row_live is None else _f64(row_live[t]).reshape(R, 1)
        out['a2_grad'] += dz.T @ (hs[t] * live)
        out['dbias_tiles'] += _tile_sums(dz)
        if obs is not None:
            out['enc_dwt'] += _f64(obs[t]).reshape(R, -1).T @ dz
    out['dh'] = dh
    out['dbias_cols'] = out['dz'].sum((0, 1))
    if obs is not None:
        out['enc_db'] = out['dbias_cols'].copy()
    return out


def mlp_window_backward(obs, enc_wt, enc_bias, h, dhead, w_heads, a2):
    """obs: T dense observations (R, obs_dim), enc_wt (obs_dim, H) = affine1.weight^T, enc_bias (H,), h (T, R, H), dhead (T, R, OT),
    w_heads (OT, H), a2 (H, H).  Everything is taken to float64.  Returns a dict: x1, dz, de (T, R, H), dbias_cols (H,) the column
    sum of dz, dbias_tiles (ceil(T R / 64), H) the tiles of the window's T x R rows, a2_grad (H, H), enc_dwt (obs_dim, H), enc_db."""
    h, dhead, w_heads, a2, enc_wt = _f64(h), _f64(dhead), _f64(w_heads), _f64(a2), _f64(enc_wt)
    T, R, H = h.shape
    ob = np.stack([_f64(o).reshape(R, -1) for o in obs])
    x1 = np.tanh(ob @ enc_wt + _f64(enc_bias))
    dz = (dhead @ w_heads) * (1.0 - h * h)
    de = (dz @ a2 + dz) * (1.0 - x1 * x1)
    flat = lambda a: a.reshape(T * R, -1)
    return dict(x1=x1, dz=dz, de=de, dbias_cols=dz.sum((0, 1)), dbias_tiles=_tile_sums(flat(dz)), a2_grad=flat(dz).T @ flat(x1),
                enc_dwt=flat(ob).T @ flat(de), enc_db=de.sum((0, 1)))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def make_rnn_window(seed, T, E, N, H, OT, collect=False, h_last='slot'):
    """Synthetic float32 records of a window of the tanh recurrence (numpy): hs = tanh of normals — T + 1 slots with h_last='slot',
    T slots and a separate `h_last` buffer with 'separate' —, random dhead and a terminal dh, weights scaled by H ** -0.5.
    collect: row_live / row_keep as bptt_window_ref.collection_cuts makes them."""
    assert h_last in ('slot', 'separate')
    rng = np.random.default_rng(seed)
    R = E * N
    rn = lambda *s: rng.standard_normal(s)
    slots = T + 1 if h_last == 'slot' else T
    w = dict(T=T, E=E, N=N, H=H, OT=OT, a2=_f32(rn(H, H) / H ** 0.5), w_heads=_f32(rn(OT, H) / H ** 0.5),
             hs=_f32(np.tanh(rn(slots, R, H))), h_last=_f32(np.tanh(rn(R, H))) if h_last == 'separate' else None,
             dhead=_f32(rn(T, R, OT)), dh=_f32(rn(R, H)), row_live=None, row_keep=None)
    if collect:
        w['row_live'], w['row_keep'], _ = collection_cuts(rng, T, E, N)
    return w


def rnn_reference_of(w, obs=None, detach_gap=0):
    """rnn_window_backward on a make_rnn_window dict"""
    return rnn_window_backward(w['hs'], w['h_last'], w['dhead'], w['w_heads'], w['a2'], w['dh'], row_live=w['row_live'],
                               row_keep=w['row_keep'], detach_gap=detach_gap, obs=obs)


def make_mlp_window(seed, T, E, N, H, OT, obs_dim):
    """Synthetic float32 records of a window of models.MLP (numpy): h = tanh of normals, random dhead, the encoder's Wt (obs_dim, H)
    scaled by 0.3 and its bias by 0.1, a2 / w_heads scaled by H ** -0.5."""
    rng = np.random.default_rng(seed)
    R = E * N
    rn = lambda *s: rng.standard_normal(s)
    return dict(T=T, E=E, N=N, H=H, OT=OT, a2=_f32(rn(H, H) / H ** 0.5), w_heads=_f32(rn(OT, H) / H ** 0.5),
                enc_wt=_f32(rn(obs_dim, H) * 0.3), enc_bias=_f32(rn(H) * 0.1), h=_f32(np.tanh(rn(T, R, H))), dhead=_f32(rn(T, R, OT)))


def mlp_reference_of(w, obs):
    """mlp_window_backward on a make_mlp_window dict"""
    return mlp_window_backward(obs, w['enc_wt'], w['enc_bias'], w['h'], w['dhead'], w['w_heads'], w['a2'])


def rnn_errors(want, dz, dh, parts, parts0, a2_grad=None, a2_grad0=None):
    """The figures of one ic3_rnn_backward window (or chain of windows) against `want` (rnn_window_backward): every slot of dz, dh,
    the partials' column sum on top of their pre-fill parts0, every partial row against dbias_tiles where there is one partial per
    tile, and a2_grad on top of its pre-fill."""
    errs = dict(dz=rel_err(dz, want['dz']), dh=rel_err(dh, want['dh']),
                dbias_cols=rel_err(_f64(parts).sum(0), _f64(parts0).sum(0) + want['dbias_cols']))
    if parts.shape[0] == want['dbias_tiles'].shape[0]:
        errs['dbias_tiles'] = rel_err(parts, _f64(parts0) + want['dbias_tiles'])
    if a2_grad is not None:
        errs['a2_grad'] = rel_err(a2_grad, _f64(a2_grad0) + want['a2_grad'])
    return errs


def mlp_errors(want, x1, dz, de, parts, a2_grad, a2_grad0, windows=1):
    """The figures of one ic3_mlp_backward window against `want` (mlp_window_backward): the three rings, the partials' column sum
    (the call writes them), every partial row where there is one per tile, a2_grad on top of its pre-fill (`windows` calls added)."""
    errs = dict(x1=rel_err(x1, want['x1']), dz=rel_err(dz, want['dz']), de=rel_err(de, want['de']),
                dbias_cols=rel_err(_f64(parts).sum(0), want['dbias_cols']))
    if parts.shape[0] == want['dbias_tiles'].shape[0]:
        errs['dbias_tiles'] = rel_err(parts, want['dbias_tiles'])
    errs['a2_grad'] = rel_err(a2_grad, _f64(a2_grad0) + windows * want['a2_grad'])
    return errs


def check(case, errs):
    """bptt_window_ref.check for the tanh windows: print every figure (worst |got - ref| / max(1, max |ref|) per quantity), then hold
    each to its bar from tanh_window_bars.BARS (4 x the measured figure, never above 1e-5: profiles/r13/tanh_window_errors.txt).
    IC3_TANH_ERRORS_OUT=<file>: the figures are appended there as JSON lines as well (how the committed figures were taken)."""
    import json
    import os
    from tanh_window_bars import BARS
    for k in sorted(errs):
        print("tanh-window %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_TANH_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)
