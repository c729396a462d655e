"""TEST INFRASTRUCTURE: the float64 reference of the non-recurrent CommNet module's window backward (ic3_commnet_backward,
include/ic3_rollout.h) — a closed-form backward over the recorded steps, numpy only, shared by the host-build and the GPU tests of
that call (and itself checked against torch float64 autograd through a transcription of the module's generic forward:
tests/test_commnet_window_ref_cpu.py).  The sibling of tanh_window_ref.py.  Nothing under ic3net_amd/ imports this.

Per step, with enc = obs @ Wt + b_enc, x = h_0 = tanh(enc) and M the (symmetric) mixing matrix of the step's masks:
    h_{i+1} = tanh(x + h_i F_i^T + M(h_i) C_i^T + b_i)      i = 0 .. P - 1          (comm_zero: without the C term)
    dh_P = dhead @ w_heads
    dz_i = dh_{i+1} (1 - h_{i+1}^2);  dF_i = dz_i^T h_i;  dC_i = dz_i^T M(h_i);  d b_i = column sums of dz_i
    dh_i = dz_i F_i + M(dz_i C_i)
    de = (sum_i dz_i + dh_0)(1 - h_0^2);  encoder: dWt = obs^T de, db = column sums of de;  heads: dW = dhead^T h_P, db = column sums
No state crosses a step: the window is the sum over its steps."""
import numpy as np

from bptt_window_ref import mix, rel_err  # noqa: F401  (re-exported: the tests take them from here)


def _f64(a):
    return np.asarray(a, np.float64)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def window_backward(obs, enc_wt, enc_bias, f_w, c_w, bias, w_heads, dhead, E, N, alive=None, gate=None, mode_avg=True,
                    comm_zero=False):
    """obs: T dense observations (R, obs_dim) — or `enc` rows when enc_wt is None —, enc_wt (obs_dim, H), enc_bias (H,), f_w / c_w:
    lists of P (H, H) weights as stored (out, in), bias (P, H) = C_i.bias + f_i.bias, w_heads (OT, H), dhead (T, R, OT), alive / gate
    (T, E, N) or None.  Everything is taken to float64.  Returns a dict: h_pass (P + 1, T, R, H), dz (P, T, R, H), dh0, de (T, R, H),
    per pass f_grad, c_grad (H, H) and bias_cols (H,) as lists, heads_w (OT, H), heads_b (OT,), and with enc_wt: enc_dwt, enc_db."""
    dhead, w_heads, bias = _f64(dhead), _f64(w_heads), _f64(bias)
    F, Cw = [_f64(w) for w in f_w], [_f64(w) for w in c_w]
    P = len(F)
    T, R, _ = dhead.shape
    assert R == E * N
    ob = np.stack([_f64(o).reshape(R, -1) for o in obs])
    enc = ob if enc_wt is None else ob @ _f64(enc_wt) + _f64(enc_bias)
    H = enc.shape[-1]
    al = lambda t: None if alive is None else np.asarray(alive)[t]
    gt = lambda t: None if gate is None else np.asarray(gate)[t]

    def M(v, t):                                                # (R, H) -> (R, H)
        if comm_zero:
            return np.zeros_like(v)
        return mix(v.reshape(E, N, H), al(t), gt(t), mode_avg).reshape(R, H)

    h = np.zeros((P + 1, T, R, H))
    h[0] = np.tanh(enc)
    for i in range(P):
        for t in range(T):
            h[i + 1, t] = np.tanh(h[0, t] + h[i, t] @ F[i].T + M(h[i, t], t) @ Cw[i].T + bias[i])
    out = dict(h_pass=h, dz=np.zeros((P, T, R, H)), f_grad=[None] * P, c_grad=[None] * P, bias_cols=[None] * P)
    dh = dhead @ w_heads
    for i in range(P - 1, -1, -1):
        dz = dh * (1.0 - h[i + 1] ** 2)
        out['dz'][i] = dz
        out['f_grad'][i] = np.einsum('tro,tri->oi', dz, h[i])
        out['c_grad'][i] = sum(dz[t].T @ M(h[i, t], t) for t in range(T))
        out['bias_cols'][i] = dz.sum((0, 1))
        dh = np.stack([dz[t] @ F[i] + M(dz[t] @ Cw[i], t) for t in range(T)])
    out['dh0'] = dh
    out['de'] = (out['dz'].sum(0) + dh) * (1.0 - h[0] ** 2)
    out['heads_w'] = np.einsum('tro,trh->oh', dhead, h[P])
    out['heads_b'] = dhead.sum((0, 1))
    if enc_wt is not None:
        out['enc_dwt'] = np.einsum('trk,trh->kh', ob, out['de'])
        out['enc_db'] = out['de'].sum((0, 1))
    return out


def make_masks(rng, T, E, N, dead=0.0, gated=0.0, min_live=2):
    """alive / gate (T, E, N) int32: an agent is dead with probability `dead`, gated off with `gated`; every env keeps at least
    `min_live` live agents (avg mode divides by n_alive - 1), checked here."""
    alive = (rng.random((T, E, N)) >= dead).astype(np.int32)
    for t in range(T):
        for e in range(E):
            while alive[t, e].sum() < min(min_live, N):
                alive[t, e, rng.integers(N)] = 1
    gate = (rng.random((T, E, N)) >= gated).astype(np.int32)
    assert (alive.sum(2) >= min(min_live, N)).all()
    return alive, gate


def make_weights(seed, H, P, OT, obs_dim, share=False):
    """Synthetic float32 weights of the module: the encoder's Wt (obs_dim, H) scaled by 0.3 and its bias by 0.1, F_i / C_i / w_heads
    scaled by H ** -0.5 (C by a further 0.5: the mixed vector is a sum over agents), the summed biases by 0.1; share: one F, one C."""
    rng = np.random.default_rng(seed)
    rn = lambda *s: rng.standard_normal(s)
    f_w = [_f32(rn(H, H) / H ** 0.5) for _ in range(1 if share else P)] * (P if share else 1)
    c_w = [_f32(0.5 * rn(H, H) / H ** 0.5) for _ in range(1 if share else P)] * (P if share else 1)
    b = _f32(rn(1 if share else P, H) * 0.1)
    return dict(H=H, P=P, OT=OT, enc_wt=_f32(rn(obs_dim, H) * 0.3), enc_bias=_f32(rn(H) * 0.1), f_w=f_w, c_w=c_w,
                bias=_f32(np.repeat(b, P, 0)) if share else b, w_heads=_f32(rn(OT, H) / H ** 0.5))


def reference_of(w, obs, dhead, E, N, alive=None, gate=None, mode_avg=True, comm_zero=False):
    """window_backward on a make_weights dict"""
    return window_backward(obs, w['enc_wt'], w['enc_bias'], w['f_w'], w['c_w'], w['bias'], w['w_heads'], dhead, E, N, alive=alive,
                           gate=gate, mode_avg=mode_avg, comm_zero=comm_zero)


def entry_errors(o, want, T, R):
    """The figures of one ic3_commnet_backward window (or windows / chunks summed onto the same gradients) against `want`
    (window_backward).  o: enc_dwt, enc_db, the gradients added to (lists f_grad / c_grad / bias_grad per pass, heads_w, heads_b) with
    their pre-fills in o['pre'] (float64), and — compared when one chunk held the whole window, o['chunks'] == 1 — the rings h_pass,
    de, dz (the first pass's, the last one written) and dh (dh_0)."""
    P, H = len(o['f_grad']), o['enc_dwt'].shape[-1]
    errs = dict(enc_dwt=rel_err(o['enc_dwt'], want['enc_dwt']), enc_db=rel_err(o['enc_db'], want['enc_db']),
                heads_w=rel_err(o['heads_w'], o['pre']['heads_w'] + want['heads_w']),
                heads_b=rel_err(o['heads_b'], o['pre']['heads_b'] + want['heads_b']))
    for k, wk in (('f_grad', 'f_grad'), ('c_grad', 'c_grad'), ('bias_grad', 'bias_cols')):
        errs[k] = max(rel_err(o[k][i], o['pre'][k][i] + want[wk][i]) for i in range(P))
    if o['chunks'] == 1:
        errs['h_pass'] = rel_err(o['h_pass'], want['h_pass'].reshape(P + 1, T * R, H))
        errs['de'] = rel_err(o['de'], want['de'].reshape(-1, H))
        errs['dz_first'] = rel_err(o['dz'], want['dz'][0].reshape(-1, H))
        errs['dh0'] = rel_err(o['dh'], want['dh0'].reshape(-1, H))
    return errs


def check(case, errs):
    """Print every figure (worst |got - ref| / max(1, max |ref|) per quantity), then hold each to its bar from
    commnet_window_bars.BARS (4 x the measured figure, never above 1e-5: profiles/r15/commnet_window_errors.txt).
    IC3_COMMNET_ERRORS_OUT=<file>: the figures are appended there as JSON lines as well (how the committed figures were taken)."""
    import json
    import os
    from commnet_window_bars import BARS
    for k in sorted(errs):
        print("commnet-window %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_COMMNET_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)
