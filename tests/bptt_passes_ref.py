"""TEST INFRASTRUCTURE: the float64 reference of a recurrent policy with comm_passes = P > 1 over a window — forward and backward,
numpy only, written from the reference's comm.py:179-218 (per pass: the masked communication sum of the CURRENT hidden state, C_i,
inp = x + c, the LSTM cell on (hidden, cell)), shared by the host-build and the GPU tests of ic3_policy_forward on an ic3_policy_record and
ic3_bptt_backward on an ic3_bptt_passes descriptor (include/ic3_rollout.h) and itself checked against torch float64 autograd through P chained LSTMCells:
tests/test_bptt_passes_ref_cpu.py.  Nothing under ic3net_amd/ imports this.

Forward of pass i of a step, on x = encoder(obs) + encoder.bias (R, H) and the state (h, c) the previous pass (step) left:
    inp = x + C_i.bias + M(h) @ C_i.weight^T;  pre = [inp | h] @ [W_ih | W_hh]^T + b;  (i, f, g, o) = activated(pre)
    c' = f c + i g;  h' = o tanh(c')
Backward, t = T - 1 .. 0 and i = P - 1 .. 0, with the records gates[i][t], hs[i][t], cs[i][t] (the state ENTERING pass i of step t):
    last  = i == P - 1;  det = last and detach_gap > 0 and (t_first + t + 1) % detach_gap == 0
    dh_t  = (0 if det else dh) + (dhead[t] @ w_heads if last else 0);  dc_in = 0 if det else dc
    tc = tanh(f cp + i g);  dct = dc_in + dh_t o (1 - tc^2);  dgates = [dct g i (1-i) | dct cp f (1-f) | dct i (1-g^2) | dh_t tc o (1-o)]
    dc = dct f;  dxh = dgates @ [W_ih | W_hh] = [d inp | d h_direct];  dh = d h_direct + M_t(d inp @ C_i.weight)   (comm_zero: no M term)
    dC_i += d inp^T @ M_t(hs[i][t]);  dC_i.bias += column sums of d inp;  bias rows of pass i += column sums of dgates per 64-row tile
    encoder: dWt += obs_t^T @ d inp, db += column sums of d inp (every pass);  LSTM: dW += [inp[i][t] | hs[i][t]]^T @ dgates
M_t: the (symmetric) mixing matrix of step t's alive / gate masks — the same for every pass of the step."""
import numpy as np

from bptt_window_ref import TILE, activated, mix, rel_err   # noqa: F401  (rel_err: re-exported to the tests)

f64 = lambda a: np.asarray(a, np.float64)


def pass_forward(x, h, c, c_weight, c_bias, w_ih, w_hh, bias, E, N, alive=None, gate=None, mode_avg=True, comm_zero=False):
    """One communication pass (comm.py:181-218) on E envs of N agents: x (R, H) = encoder(obs) + encoder.bias, (h, c) (R, H) entering.
    Returns the activated gates (R, 4H), inp (R, H), h', c'."""
    x, h, c = f64(x), f64(h), f64(c)
    R, H = h.shape
    comm = np.zeros((R, H)) if comm_zero else mix(h.reshape(E, N, H), alive, gate, mode_avg).reshape(R, H)
    inp = x + f64(c_bias) + comm @ f64(c_weight).T
    a = activated(np.concatenate([inp, h], 1) @ np.concatenate([f64(w_ih), f64(w_hh)], 1).T + f64(bias))
    i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    c1 = f * c + i * g
    return a, inp, o * np.tanh(c1), c1


def window_forward(x, h0, c0, c_weights, c_biases, w_ih, w_hh, bias, E, N, alive=None, gate=None, mode_avg=True, comm_zero=False,
                   detach_gap=0, entering=None):
    """T steps of P passes from (h0, c0): x (T, R, H), c_weights / c_biases lists of P.  Returns the records gates (P, T, R, 4H),
    inp, hs, cs (P, T, R, H) (hs[i][t]: the state entering pass i of step t) and the state (h, c) leaving the window.  (detach_gap
    changes nothing in the forward: it is taken so that both directions are called alike.)  entering = (hs, cs) (T, R, H): every step
    starts from the RECORDED state instead of what the step before left — how the update re-evaluates the passes of a window."""
    x = f64(x)
    T, R, H = x.shape
    P = len(c_weights)
    rec = dict(gates=np.zeros((P, T, R, 4 * H)), inp=np.zeros((P, T, R, H)), hs=np.zeros((P, T, R, H)), cs=np.zeros((P, T, R, H)))
    h, c = f64(h0), f64(c0)
    for t in range(T):
        if entering is not None:
            h, c = f64(entering[0][t]), f64(entering[1][t])
        for i in range(P):
            rec['hs'][i, t], rec['cs'][i, t] = h, c
            rec['gates'][i, t], rec['inp'][i, t], h, c = pass_forward(
                x[t], h, c, c_weights[i], c_biases[i], w_ih, w_hh, bias, E, N, None if alive is None else alive[t],
                None if gate is None else gate[t], mode_avg, comm_zero)
    rec['h'], rec['c'] = h, c
    return rec


def window_backward(gates, hs, cs, dhead, w_heads, w_ih, w_hh, dh, dc, E, N, c_weights=None, alive=None, gate=None, detach_gap=0,
                    t_first=0, mode_avg=True, comm_zero=False, obs=None, inp=None):
    """gates (P, T, R, 4H), hs / cs (P, T, R, H), dhead (T, R, OT), dh / dc (R, H) arriving at the last step, c_weights: P of (H, H),
    alive / gate: None or T entries (E, N) / None, obs: None or T dense observations (R, obs_dim), inp: None or (P, T, R, H).
    Returns dgates (P, T, R, 4H), dxh (P, T, R, 2H), dh, dc leaving the first step, dbias_rows (P, ceil(R / 64), 4H), dcw (P, H, H),
    dcb (P, H), and with obs: enc_dwt, enc_db; with inp: dW (2H, 4H)."""
    gates, hs, cs, dhead, w_heads = f64(gates), f64(hs), f64(cs), f64(dhead), f64(w_heads)
    P, T, R, H4 = gates.shape
    H = H4 // 4
    assert R == E * N
    W = np.concatenate([f64(w_ih), f64(w_hh)], 1)               # (4H, 2H)
    dh, dc = f64(dh).copy(), f64(dc).copy()
    tiles = (R + TILE - 1) // TILE
    out = dict(dgates=np.zeros((P, T, R, 4 * H)), dxh=np.zeros((P, T, R, 2 * H)), dbias_rows=np.zeros((P, tiles, 4 * H)),
               dcw=np.zeros((P, H, H)), dcb=np.zeros((P, H)))
    if obs is not None:
        out['enc_dwt'], out['enc_db'] = np.zeros((f64(obs[0]).shape[-1], H)), np.zeros(H)
    if inp is not None:
        out['dW'] = np.zeros((2 * H, 4 * H))
    for t in range(T - 1, -1, -1):
        al = None if alive is None else alive[t]
        gt = None if gate is None else gate[t]
        for p in range(P - 1, -1, -1):
            last = p == P - 1
            det = last and detach_gap > 0 and (t_first + t + 1) % detach_gap == 0
            dh_t = (0.0 if det else dh) + (dhead[t] @ w_heads if last else 0.0)
            dc_in = 0.0 if det else dc
            i, f, g, o = gates[p, t, :, :H], gates[p, t, :, H:2 * H], gates[p, t, :, 2 * H:3 * H], gates[p, t, :, 3 * H:]
            cp = cs[p, t]
            tc = np.tanh(f * cp + i * g)
            dct = dc_in + dh_t * o * (1 - tc * tc)
            dg = np.concatenate([dct * g * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - g * g), dh_t * tc * o * (1 - o)], 1)
            out['dgates'][p, t] = dg
            dc = dct * f
            dxh = dg @ W
            out['dxh'][p, t] = dxh
            dinp, dhd = dxh[:, :H], dxh[:, H:]
            if comm_zero:
                dh = dhd
            else:
                C = f64(c_weights[p])
                dh = dhd + mix((dinp @ C).reshape(E, N, H), al, gt, mode_avg).reshape(R, H)
                out['dcw'][p] += dinp.T @ mix(hs[p, t].reshape(E, N, H), al, gt, mode_avg).reshape(R, H)
            out['dcb'][p] += dinp.sum(0)
            for w in range(tiles):
                out['dbias_rows'][p, w] += dg[TILE * w:TILE * w + TILE].sum(0)
            if obs is not None:
                out['enc_dwt'] += f64(obs[t]).reshape(R, -1).T @ dinp
                out['enc_db'] += dinp.sum(0)
            if inp is not None:
                out['dW'] += np.concatenate([f64(inp[p, t]), hs[p, t]], 1).T @ dg
    out['dh'], out['dc'] = dh, dc
    return out


def make_window(seed, T, E, N, H, OT, P, share=False, alive='none', gate='random'):
    """Synthetic float32 records of a P-pass window (numpy): activated gates from random pre-activations, random hs / cs / inp of every
    (pass, step), dhead and the terminal dh / dc, weights scaled by H ** -0.5.  share: one C for every pass (the list holds the same
    array P times).  alive: 'none', 'first_null' or 'all'; gate: 'none' or 'random'."""
    rng = np.random.default_rng(seed)
    R = E * N
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    rn = lambda *s: rng.standard_normal(s)
    cws = [f32(rn(H, H) / H ** 0.5) for _ in range(1 if share else P)]
    w = dict(T=T, E=E, N=N, H=H, OT=OT, P=P, w_ih=f32(rn(4 * H, H) / H ** 0.5), w_hh=f32(rn(4 * H, H) / H ** 0.5),
             c_weights=cws * P if share else cws, w_heads=f32(rn(OT, H) / H ** 0.5), gates=f32(activated(rn(P, T, R, 4 * H))),
             hs=f32(np.tanh(rn(P, T, R, H))), cs=f32(rn(P, T, R, H)), inp=f32(rn(P, T, R, H)), dhead=f32(rn(T, R, OT)),
             dh=f32(rn(R, H)), dc=f32(rn(R, H)))
    mask = lambda p: np.ascontiguousarray(rng.random((E, N)) < p, np.int32)
    w['alive'] = None if alive == 'none' else [None if (alive == 'first_null' and t == 0) else mask(0.8) for t in range(T)]
    w['gate'] = None if gate == 'none' else [mask(0.6) for t in range(T)]
    return w


def reference_of(w, obs=None, **kw):
    """window_backward on a make_window dict"""
    return window_backward(w['gates'], w['hs'], w['cs'], w['dhead'], w['w_heads'], w['w_ih'], w['w_hh'], w['dh'], w['dc'], w['E'], w['N'],
                           c_weights=w['c_weights'], alive=w['alive'], gate=w['gate'], obs=obs, inp=w['inp'], **kw)


def check(case, errs):
    """Print every figure (worst |got - ref| / max(1, max |ref|) per quantity), then hold each to its bar from bptt_passes_bars.BARS
    (4 x the measured figure, never above 1e-5: profiles/r18/bptt_passes_errors.txt).  IC3_BPTT_ERRORS_OUT=<file>: the figures are
    appended there as JSON lines as well (how the committed figures were taken)."""
    import json
    import os
    from bptt_passes_bars import BARS
    for k in sorted(errs):
        print("bptt-passes %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_BPTT_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)
