"""TEST INFRASTRUCTURE: what the host-build and the GPU tests of ic3_policy_step on an ic3_policy_window_record (the npasses window that
records its passes' gates, include/ic3_rollout.h) share — the float64 reference of the record and the check of the figures against
tests/window_record_bars.py.  numpy only; nothing under ic3net_amd/ imports this.

The reference is tests/bptt_passes_ref.pass_forward, run pass by pass from the window's recorded (hs[t], cs[t]), the masks of step t
and float64 encoder rows: the dense observation of the snapshot entering step t times encoder.weight in float64, plus encoder.bias
(pass_forward adds C_i.bias).  An auto-reset env whose snapshot has t == 0 starts an episode at that step: zero state at pass 0,
nobody dead, gate 0 for every pass of the step (the per-step kernel's rule)."""
import json
import os

import numpy as np

from bptt_passes_ref import pass_forward, rel_err

QUANTITIES = ('rec_gates', 'rec_inp', 'rec_h', 'rec_c')


def reference_record(P, E, N, H, obs, hs, cs, enc_w, enc_b, c_weights, c_biases, w_ih, w_hh, bias, alive, gate, fresh=None):
    """obs (T, R, obs_dim) dense rows of the state entering every step; hs, cs (T + 1, R, H) the window's record; c_weights / c_biases:
    P entries; alive / gate: T entries (E, N) or None; fresh: None or (T, E) bool.  Returns float64 gates (P, T, R, 4H), inp, h, c
    (P, T, R, H): h[i][t], c[i][t] the state ENTERING pass i of step t (i = 0: the record's, with the restarts applied)."""
    T, R = obs.shape[0], E * N
    ref = dict(gates=np.zeros((P, T, R, 4 * H)), inp=np.zeros((P, T, R, H)), h=np.zeros((P, T, R, H)), c=np.zeros((P, T, R, H)))
    for t in range(T):
        x = np.asarray(obs[t], np.float64).reshape(R, -1) @ np.asarray(enc_w, np.float64).T + np.asarray(enc_b, np.float64)
        h, c = np.asarray(hs[t], np.float64).copy(), np.asarray(cs[t], np.float64).copy()
        al, gt = alive[t], gate[t]
        if fresh is not None and fresh[t].any():
            rows = np.repeat(fresh[t], N)
            h[rows], c[rows] = 0.0, 0.0
            al = None if al is None else np.where(fresh[t][:, None], 1, np.asarray(al).reshape(E, N))
            gt = np.where(fresh[t][:, None], 0, np.ones((E, N), np.int32) if gt is None else np.asarray(gt).reshape(E, N))
        for i in range(P):
            ref['h'][i, t], ref['c'][i, t] = h, c
            ref['gates'][i, t], ref['inp'][i, t], h, c = pass_forward(x, h, c, c_weights[i], c_biases[i], w_ih, w_hh, bias, E, N, al, gt)
    return ref


def record_errors(P, H, rec, ref):
    """The four figures: worst |got - ref| / max(1, max |ref|) of the passes' gates, the inp half of their inp rows, and the (h, c)
    entering passes 1 .. P - 1.  rec: numpy gates (P, T, R, 4H), inp (P, T, R, 2H), h, c (P, T, R, H)."""
    return dict(rec_gates=rel_err(rec['gates'][:P], ref['gates']), rec_inp=rel_err(rec['inp'][:P, :, :, :H], ref['inp']),
                rec_h=rel_err(rec['h'][1:P], ref['h'][1:]), rec_c=rel_err(rec['c'][1:P], ref['c'][1:]))


def check(case, errs):
    """Print every figure, then hold each to its bar from window_record_bars.BARS (4 x the measured figure, never above 1e-5:
    profiles/r28/window_record_errors.txt).  IC3_WINDOW_RECORD_ERRORS_OUT=<file>: the figures are appended there as JSON lines as
    well (how the committed figures were taken)."""
    from window_record_bars import BARS
    for k in sorted(errs):
        print("window-record %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_WINDOW_RECORD_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)
