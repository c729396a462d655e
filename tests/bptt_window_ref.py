"""TEST INFRASTRUCTURE: the float64 reference of the LSTM window backward (ic3_bptt_backward, include/ic3_rollout.h) — a closed-form
backward over the recorded steps, numpy only, shared by the host-build and the GPU tests of that call (and itself checked against
torch float64 autograd through a consistent forward: tests/test_bptt_window_ref_cpu.py).  Nothing under ic3net_amd/ imports this.

Per step t = T-1 .. 0, with (i, f, g, o) = gates[t] the recorded ACTIVATED gates and (hs[t], cs[t]) the state that entered:
    det   = detach_gap > 0 and (t + 1) % detach_gap == 0
    dh_t  = (0 if det else dh) + dhead[t] @ w_heads
    dc_in = (0 if det else dc) * row_keep[t]
    cp = cs[t] * row_live[t];  tc = tanh(f cp + i g);  dct = dc_in + dh_t o (1 - tc^2)
    dgates[t] = [dct g i (1-i) | dct cp f (1-f) | dct i (1-g^2) | dh_t tc o (1-o)];  dc = dct f
    dxh[t] = dgates[t] @ [W_ih | W_hh] = [d inp | d h_direct]
    dh = (d h_direct + M_t(d inp @ C)) * row_keep[t-1]        (comm_zero: without the M_t term; t = 0: no factor)
    dC += d inp^T @ M_t(hs[t]);  bias row w += column sums of dgates[t][64 w : 64 w + 64]
    encoder: dWt += obs_t^T @ d inp, db += column sums of d inp;  LSTM: dW += [inp_t | row_live[t] hs[t]]^T @ dgates[t]
M_t is the (symmetric) mixing matrix of the communication step for alive[t] / gate[t] (None = ones)."""
import numpy as np

TILE = 64


def mix(x, alive, gate, mode_avg):
    """The communication step's masked mean / sum over the other agents of an env, (E, N, H) float64 -> (E, N, H):
    out_i = g_i * sum_{j != i} g_j x_j * (1 / (n_alive - 1) in avg mode when n_alive > 1), g = alive * gate."""
    E, N, _ = x.shape
    al = np.ones((E, N)) if alive is None else np.asarray(alive, np.float64).reshape(E, N)
    g = al * (np.ones((E, N)) if gate is None else np.asarray(gate, np.float64).reshape(E, N))
    S = (g[:, :, None] * x).sum(1, keepdims=True)
    n_alive = al.sum(1)
    scale = np.where(n_alive > 1, 1.0 / np.maximum(n_alive - 1, 1), 1.0) if mode_avg else np.ones(E)
    return g[:, :, None] * (S - g[:, :, None] * x) * scale[:, None, None]


def window_backward(gates, hs, cs, dhead, w_heads, w_ih, w_hh, dh, dc, E, N, c_weight=None, alive=None, gate=None,
                    row_live=None, row_keep=None, detach_gap=0, mode_avg=True, comm_zero=False, obs=None, inp=None):
    """gates (T, R, 4H), hs / cs (>= T, R, H), dhead (T, R, OT), w_heads (OT, H), w_ih / w_hh (4H, H), dh / dc (R, H) arriving at
    the last step, c_weight (H, H), alive / gate: None or lists of T entries (E, N) / None, row_live / row_keep (T, R) or None,
    obs: None or T dense observations (R, obs_dim), inp: None or (T, R, H) the recorded inp rows.  Everything is taken to float64.
    Returns a dict: dgates (T, R, 4H), dxh (T, R, 2H), dh, dc (R, H) leaving the first step, dbias_rows (ceil(R / 64), 4H), dcw
    (H, H), and with obs: enc_dwt (obs_dim, H), enc_db (H,); with inp: dW (2H, 4H)."""
    f64 = lambda a: np.asarray(a, np.float64)
    gates, hs, cs, dhead, w_heads = f64(gates), f64(hs), f64(cs), f64(dhead), f64(w_heads)
    T, R, H4 = gates.shape
    H = H4 // 4
    assert R == E * N
    W = np.concatenate([f64(w_ih), f64(w_hh)], 1)               # (4H, 2H)
    dh, dc = f64(dh).copy(), f64(dc).copy()
    C = None if comm_zero else f64(c_weight)
    tiles = (R + TILE - 1) // TILE
    out = dict(dgates=np.zeros((T, R, 4 * H)), dxh=np.zeros((T, R, 2 * H)), dbias_rows=np.zeros((tiles, 4 * H)),
               dcw=np.zeros((H, H)))
    if obs is not None:
        out['enc_dwt'], out['enc_db'] = np.zeros((f64(obs[0]).shape[-1], H)), np.zeros(H)
    if inp is not None:
        out['dW'] = np.zeros((2 * H, 4 * H))
    for t in range(T - 1, -1, -1):
        det = detach_gap > 0 and (t + 1) % detach_gap == 0
        live = np.ones((R, 1)) if row_live is None else f64(row_live[t]).reshape(R, 1)
        keep = np.ones((R, 1)) if row_keep is None else f64(row_keep[t]).reshape(R, 1)
        dh_t = (0.0 if det else dh) + dhead[t] @ w_heads
        dc_in = (0.0 if det else dc) * keep
        i, f, g, o = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:3 * H], gates[t, :, 3 * H:]
        cp = cs[t] * live
        tc = np.tanh(f * cp + i * g)
        dct = dc_in + dh_t * o * (1 - tc * tc)
        dg = np.concatenate([dct * g * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - g * g), dh_t * tc * o * (1 - o)], 1)
        out['dgates'][t] = dg
        dc = dct * f
        dxh = dg @ W
        out['dxh'][t] = dxh
        dinp, dhd = dxh[:, :H], dxh[:, H:]
        scale = f64(row_keep[t - 1]).reshape(R, 1) if (row_keep is not None and t > 0) else 1.0
        if comm_zero:
            dh = dhd * scale
        else:
            al = None if alive is None else alive[t]
            gt = None if gate is None else gate[t]
            dh = (dhd + mix((dinp @ C).reshape(E, N, H), al, gt, mode_avg).reshape(R, H)) * scale
            out['dcw'] += dinp.T @ mix(hs[t].reshape(E, N, H), al, gt, mode_avg).reshape(R, H)
        for w in range(tiles):
            out['dbias_rows'][w] += dg[TILE * w:TILE * w + TILE].sum(0)
        if obs is not None:
            out['enc_dwt'] += f64(obs[t]).reshape(R, -1).T @ dinp
            out['enc_db'] += dinp.sum(0)
        if inp is not None:
            out['dW'] += np.concatenate([f64(inp[t]), hs[t] * live], 1).T @ dg
    out['dh'], out['dc'] = dh, dc
    return out


def activated(pre):
    """(.., 4H) pre-activations -> the activated i | f | g | o record"""
    H = pre.shape[-1] // 4
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    return np.concatenate([sig(pre[..., :2 * H]), np.tanh(pre[..., 2 * H:3 * H]), sig(pre[..., 3 * H:])], -1)


def collection_cuts(rng, T, E, N, p_fresh=0.3, p_cut=0.2):
    """row_live / row_keep (T, E * N) float32 and the per-step `fresh` env masks (T, E) as the product's collection mode makes them:
    an env starting an episode at slot t has row_live[t] = 0 and nothing crosses into it (row_keep[t - 1] = 0); row_keep has further
    zeros (detach points).  Callers give fresh envs alive = 1, gate = 0 at that slot."""
    fresh = rng.random((T, E)) < p_fresh
    live = 1.0 - fresh
    keep = (rng.random((T, E)) >= p_cut).astype(np.float64)
    keep[:-1] *= live[1:]
    rep = lambda a: np.ascontiguousarray(np.repeat(a, N, axis=1), np.float32)
    return rep(live), rep(keep), fresh


def rel_err(got, want):
    """worst |got - want| / max(1, max |want|)"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, np.abs(want).max()))


def make_window(seed, T, E, N, H, OT, collect=False, alive='none', gate='random'):
    """Synthetic float32 records of a window (numpy): activated gates from random pre-activations, random hs / cs / inp / dhead and
    terminal dh / dc, weights scaled by H ** -0.5.  alive: 'none' (NULL), 'first_null' (entry 0 None, later ones set) or 'all';
    gate: 'none' or 'random' (hard attention).  collect: row_live / row_keep as collection_cuts makes them, fresh envs with
    alive = 1, gate = 0 (needs gate='random')."""
    rng = np.random.default_rng(seed)
    R = E * N
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    rn = lambda *s: rng.standard_normal(s)
    w = dict(T=T, E=E, N=N, H=H, OT=OT,
             w_ih=f32(rn(4 * H, H) / H ** 0.5), w_hh=f32(rn(4 * H, H) / H ** 0.5), c_weight=f32(rn(H, H) / H ** 0.5),
             w_heads=f32(rn(OT, H) / H ** 0.5), gates=f32(activated(rn(T, R, 4 * H))), hs=f32(np.tanh(rn(T, R, H))), cs=f32(rn(T, R, H)),
             inp=f32(rn(T, R, H)), dhead=f32(rn(T, R, OT)), dh=f32(rn(R, H)), dc=f32(rn(R, H)), row_live=None, row_keep=None)
    mask = lambda p: np.ascontiguousarray(rng.random((E, N)) < p, np.int32)
    w['alive'] = None if alive == 'none' else [None if (alive == 'first_null' and t == 0) else mask(0.8) for t in range(T)]
    w['gate'] = None if gate == 'none' else [mask(0.6) for t in range(T)]
    if collect:
        assert w['gate'] is not None
        w['row_live'], w['row_keep'], fresh = collection_cuts(rng, T, E, N)
        for t in range(T):
            w['gate'][t][fresh[t]] = 0
            if w['alive'] is not None and w['alive'][t] is not None:
                w['alive'][t][fresh[t]] = 1
    return w


def reference_of(w, obs=None, **kw):
    """window_backward on a make_window dict"""
    return window_backward(w['gates'], w['hs'], w['cs'], w['dhead'], w['w_heads'], w['w_ih'], w['w_hh'], w['dh'], w['dc'], w['E'], w['N'],
                           c_weight=w['c_weight'], alive=w['alive'], gate=w['gate'], row_live=w['row_live'], row_keep=w['row_keep'],
                           obs=obs, inp=w['inp'], **kw)


def check(case, errs):
    """Print every figure (worst |got - ref| / max(1, max |ref|) per quantity), then hold each to its bar from bptt_window_bars.BARS
    (4 x the larger of the host build's and the GPU's measured figure, never above 1e-5: profiles/r09/bptt_window_errors.txt).
    IC3_BPTT_ERRORS_OUT=<file>: the figures are appended there as JSON lines as well (how the committed figures were taken)."""
    import json
    import os
    from bptt_window_bars import BARS
    for k in sorted(errs):
        print("bptt-window %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_BPTT_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)


# ---- one gate launch (ic3_lstm_gates_backward_given) -------------------------------------------------------------------------------
GATE_SHAPES = [(64, 150), (64, 128), (64, 37), (128, 64 * 70 + 17), (128, 640)]
# the forms of the call the window issues: the collection-mode cuts on / off x dh / dc NULL (a detach point).  row_keep scales dc, so
# the launch takes it only with dc: the cut forms without dc carry row_live alone.
GATE_FORMS = [dict(cut=False, dh=True, dc=True), dict(cut=True, dh=True, dc=True), dict(cut=False, dh=False, dc=True),
              dict(cut=True, dh=False, dc=True), dict(cut=False, dh=True, dc=False), dict(cut=True, dh=True, dc=False),
              dict(cut=False, dh=False, dc=False), dict(cut=True, dh=False, dc=False)]


def make_gate_step(seed, H, R, OT):
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    rn = lambda *s: rng.standard_normal(s)
    return dict(H=H, R=R, OT=OT, w_ih=f32(rn(4 * H, H) / H ** 0.5), w_hh=f32(rn(4 * H, H) / H ** 0.5), gates=f32(activated(rn(R, 4 * H))),
                c_prev=f32(rn(R, H)), h_prev=f32(rn(R, H)), dh=f32(rn(R, H)), dc=f32(rn(R, H)), dhead=f32(rn(R, OT)),
                w_heads=f32(rn(OT, H) / H ** 0.5), live=f32(rng.random(R) < 0.7), keep=f32(rng.random(R) < 0.6),
                parts0=f32(rn((R + 63) // 64, 4 * H)))


def gate_step_reference(s, form):
    """dgates, dc_prev, dxh, the tile rows of the bias partials' increment — float64 closed form of one launch in `form`."""
    f64 = lambda a: np.asarray(a, np.float64)
    H, R = s['H'], s['R']
    a = f64(s['gates'])
    i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    cp = f64(s['c_prev']) * (f64(s['live'])[:, None] if form['cut'] else 1.0)
    dcv = (f64(s['dc']) if form['dc'] else 0.0) * (f64(s['keep'])[:, None] if (form['cut'] and form['dc']) else 1.0)
    dhv = (f64(s['dh']) if form['dh'] else 0.0) + f64(s['dhead']) @ f64(s['w_heads'])
    tc = np.tanh(f * cp + i * g)
    dct = dcv + dhv * o * (1 - tc * tc)
    dg = np.concatenate([dct * g * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - g * g), dhv * tc * o * (1 - o)], 1)
    rows = np.stack([dg[TILE * w:TILE * w + TILE].sum(0) for w in range((R + TILE - 1) // TILE)])
    return dg, dct * f, dg @ np.concatenate([f64(s['w_ih']), f64(s['w_hh'])], 1), rows
