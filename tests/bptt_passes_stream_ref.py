"""TEST INFRASTRUCTURE: the float64 reference of the comm_passes = P > 1 window backward in COLLECTION mode — the window is T consecutive
slots of E streams of episodes, and the recurrence is cut where an episode ends or starts inside it.  numpy only, built on the
lock-step multi-pass reference tests/bptt_passes_ref.py (its pass_forward / window_forward, mix and activated, and its window_backward
applied to ONE slot at a time), shared by the host-build and the GPU tests of ic3_bptt_backward on an ic3_bptt_passes descriptor with
row_keep / keep_before, and itself checked against torch float64 autograd: tests/test_bptt_passes_stream_ref_cpu.py.  Nothing under
ic3net_amd/ imports this.

The cuts, as statements about slots (not about launches):
    fresh[t, e] = env e STARTS an episode at slot t.  Its step runs on a zero state — (h, c) entering pass 0 are zeros, whatever the
        record holds — with nobody dead and, where the window has gates at all, every agent gated off, in every pass of that step.
        The zeros are constants of the forward: nothing is multiplied into the gradient on the way back out of the slot.
    keep[t, e]  = the state LEAVING slot t reaches slot t + 1 with its gradient.  dL/d(h, c) of the state leaving slot t — what the
        later slots (or the later window) send back — is multiplied by keep[t] before slot t's passes see it.
So a slot's backward is the lock-step backward of a one-step window (bptt_passes_ref.window_backward, T = 1, no detach point) on
(keep[t] dh, keep[t] dc), and the window is the slots chained last to first; what leaves slot 0 is returned as it is (keep of the slot
in front belongs to the earlier window).  A chunk of a window is the same function on the chunk's slots: the caller multiplies what
the chunk returns by nothing — the NEXT call's keep[t] does it."""
import numpy as np

import bptt_passes_ref as base
from bptt_passes_ref import activated, mix, pass_forward      # noqa: F401  (the pieces this reference is made of)

f64 = base.f64
rel_err = base.rel_err


def rows(flags, N):
    """(T, E) flags -> (T, E * N, 1) float64 row factors"""
    return np.repeat(f64(flags), N, axis=1)[:, :, None]


def cut_masks(alive, gate, fresh, N):
    """The T steps' masks with the starting envs' rows set: alive -> ones, gate -> zeros.  None (no mask at all) stays None; a None
    entry of a list counts as all ones first."""
    fr = np.asarray(fresh, bool)
    T, E = fr.shape
    ones = np.ones((E, N), np.int32)

    def cut(ms, value):
        if ms is None:
            return None
        return [np.ascontiguousarray(np.where(fr[t][:, None], value, ones if ms[t] is None else ms[t]), np.int32) for t in range(T)]
    return cut(alive, 1), cut(gate, 0)


def entering(hs_rec, cs_rec, fresh, N):
    """The recorded (h, c) entering every slot (T, R, H) with the starting envs' rows zeroed (copies, float64)."""
    live = 1.0 - rows(fresh, N)
    return f64(hs_rec) * live, f64(cs_rec) * live


def stream_forward(x, hs_rec, cs_rec, fresh, c_weights, c_biases, w_ih, w_hh, bias, E, N, alive=None, gate=None, mode_avg=True,
                   comm_zero=False):
    """The P passes of every slot re-evaluated from the recorded entering state, with the starting envs on zeros and their masks cut:
    the records of bptt_passes_ref.window_forward (gates, inp, hs, cs: (P, T, R, .))."""
    al, gt = cut_masks(alive, gate, fresh, N)
    h_in, c_in = entering(hs_rec, cs_rec, fresh, N)
    return base.window_forward(x, h_in[0], c_in[0], c_weights, c_biases, w_ih, w_hh, bias, E, N, alive=al, gate=gt, mode_avg=mode_avg,
                               comm_zero=comm_zero, entering=(h_in, c_in))


def stream_backward(gates, hs, cs, hs_rec, cs_rec, fresh, keep, dhead, w_heads, w_ih, w_hh, dh, dc, E, N, c_weights=None, alive=None,
                    gate=None, mode_avg=True, comm_zero=False, obs=None, inp=None):
    """gates (P, T, R, 4H), hs / cs (P, T, R, H): the records of the passes (pass 0's entering state is NOT taken from them but formed
    here: hs_rec / cs_rec (T, R, H) with the starting envs zeroed); fresh, keep (T, E); alive / gate: the RAW masks (cut here);
    dh / dc (R, H): what the later window sends back, BEFORE keep[T - 1].  Returns what bptt_passes_ref.window_backward returns, for
    the whole window; dh / dc are what leaves slot 0 (not multiplied by any keep)."""
    gates, hs, cs = f64(gates), f64(hs).copy(), f64(cs).copy()
    P, T, R, H4 = gates.shape
    hs[0], cs[0] = entering(hs_rec, cs_rec, fresh, N)
    al, gt = cut_masks(alive, gate, fresh, N)
    kp = rows(keep, N)
    dh, dc = f64(dh), f64(dc)
    total = None
    for t in range(T - 1, -1, -1):
        one = base.window_backward(gates[:, t:t + 1], hs[:, t:t + 1], cs[:, t:t + 1], f64(dhead)[t:t + 1], w_heads, w_ih, w_hh,
                                   kp[t] * dh, kp[t] * dc, E, N, c_weights=c_weights, alive=None if al is None else al[t:t + 1],
                                   gate=None if gt is None else gt[t:t + 1], mode_avg=mode_avg, comm_zero=comm_zero,
                                   obs=None if obs is None else obs[t:t + 1], inp=None if inp is None else f64(inp)[:, t:t + 1])
        dh, dc = one.pop('dh'), one.pop('dc')
        if total is None:
            total = {k: (np.zeros((P, T) + v.shape[2:]) if k in ('dgates', 'dxh') else np.zeros_like(v)) for k, v in one.items()}
        for k, v in one.items():
            if k in ('dgates', 'dxh'):
                total[k][:, t] = v[:, 0]
            else:
                total[k] += v
    total['dh'], total['dc'] = dh, dc
    return total


def product_cuts(T, E, starts, extra_zero=()):
    """fresh / keep (T, E) of the shape a rollout produces: starts = [(t, e)] episode starts, keep[t - 1, e] = 0 in front of each
    (an episode ended there) plus extra_zero = [(t, e)] (detach points of an env's own step counter)."""
    fresh, keep = np.zeros((T, E), bool), np.ones((T, E), bool)
    for t, e in starts:
        fresh[t, e] = True
        if t > 0:
            keep[t - 1, e] = False
    for t, e in extra_zero:
        keep[t, e] = False
    return fresh, keep


def independent_cuts(seed, T, E, q=0.25):
    """fresh and keep drawn independently of each other, about a quarter set / cleared: every factor's slot is pinned on its own"""
    rng = np.random.default_rng(seed)
    return rng.random((T, E)) < q, rng.random((T, E)) >= q


def check(case, errs):
    """bptt_passes_ref.check against the bars of this family (bptt_passes_stream_bars.BARS: 4 x the measured figure, never above 1e-5,
    profiles/r19/bptt_passes_stream_errors.txt); every figure is printed first, IC3_BPTT_ERRORS_OUT=<file> collects them."""
    import json
    import os
    from bptt_passes_stream_bars import BARS
    for k in sorted(errs):
        print("bptt-passes-stream %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_BPTT_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)
