"""TEST INFRASTRUCTURE: the bars of the hid-256 tanh window-backward tests (tests/test_host_tanh_window_h256_cpu.py,
tests/test_tanh_window_h256_gpu.py), case -> quantity -> bar: 4 x the measured worst |got - ref| / max(1, max |ref|) against the
float64 window backwards of tests/tanh_window_ref.py for the committed seeds (host cases: measured on the host build; gpu cases: on
the MI355X), never above 1e-5 — the figures behind every entry are in profiles/r14/tanh_window_h256_errors.txt.  check() is
tanh_window_ref.check on these bars."""
CAP = 1e-5

BARS = {
    'host/rnn-A-h256-T3-gap2': {
        'dz': 5.44e-07,
        'dh': 1.59e-06,
        'dbias_cols': 5.78e-07,
        'dbias_tiles': 4.62e-07,
        'a2_grad': 6.04e-07,
        'enc_dwt': 1.10e-06,
        'enc_db': 9.60e-07,
    },
    'host/rnn-B-h256-collect-two-windows': {
        'dz': 1.83e-06,
        'dh': 1.85e-06,
        'dbias_cols': 1.39e-06,
        'dbias_tiles': 1.34e-06,
        'a2_grad': 8.96e-07,
        'enc_dwt': 2.28e-06,
        'enc_db': 1.91e-06,
    },
    'host/rnn-C-h256-T3-per-step-OT16-h-last': {
        'dz': 2.03e-06,
        'dh': 3.30e-06,
        'dbias_cols': 1.13e-06,
        'dbias_tiles': 1.37e-06,
        'a2_grad': 1.26e-06,
        'enc_dwt': 1.22e-06,
        'enc_db': 1.20e-06,
    },
    'host/mlp-A-h256-T2': {
        'x1': 9.83e-07,
        'dz': 3.34e-07,
        'de': 1.28e-06,
        'dbias_cols': 6.45e-07,
        'dbias_tiles': 4.69e-07,
        'a2_grad': 6.44e-07,
        'enc_dwt_ordered': 1.52e-06,
        'enc_db_ordered': 1.60e-06,
        'enc_dwt': 1.52e-06,
        'enc_db': 1.60e-06,
    },
    'host/mlp-B-h256-T2-table-two-windows': {
        'x1': 1.06e-06,
        'dz': 3.85e-07,
        'de': 1.78e-06,
        'dbias_cols': 5.30e-07,
        'dbias_tiles': 4.67e-07,
        'a2_grad': 7.13e-07,
        'enc_dwt_ordered': 1.12e-06,
        'enc_db_ordered': 1.97e-06,
        'enc_dwt': 1.12e-06,
        'enc_db': 1.97e-06,
    },
    'host/wgrad-h256-Q203-row-live': {
        'a2_grad': 6.42e-07,
        'a2_grad_accumulated': 6.42e-07,
    },
    'gpu/rnn-h256-pp-hard-E131-T5-gap2-h-last': {
        'dz': 5.32e-07,
        'dh': 1.64e-06,
        'dbias_cols': 4.95e-07,
        'dbias_tiles': 5.37e-07,
        'a2_grad': 9.11e-07,
        'enc_dwt': 1.19e-06,
        'enc_db': 1.15e-06,
    },
    'gpu/rnn-h256-tj-easy-E130-T4-collect-per-step-OT16': {
        'dz': 1.81e-06,
        'dh': 2.76e-06,
        'dbias_cols': 6.57e-07,
        'dbias_tiles': 8.76e-07,
        'a2_grad': 1.12e-06,
        'enc_dwt': 8.91e-07,
        'enc_db': 6.51e-07,
    },
    'gpu/rnn-h256-tj-hard-E67-two-windows-T3-collect': {
        'dz': 2.38e-06,
        'dh': 2.99e-06,
        'dbias_cols': 1.43e-06,
        'dbias_tiles': 9.05e-07,
        'a2_grad': 1.24e-06,
        'enc_dwt': 1.20e-06,
        'enc_db': 1.27e-06,
    },
    'gpu/rnn-h256-pp-n3-E5700-T2-two-tiles-a-workgroup': {
        'dz': 2.14e-06,
        'dh': 2.67e-06,
        'dbias_cols': 7.67e-07,
        'a2_grad': 1.77e-06,
        'enc_dwt': 8.63e-07,
        'enc_db': 1.19e-06,
    },
    'gpu/rnn-h256-pp-n3-E9-T1-gap1-OT1-no-a2': {
        'dz': 1.17e-07,
        'dh': 5.36e-07,
        'dbias_cols': 1.65e-07,
        'dbias_tiles': 1.65e-07,
        'enc_dwt': 3.95e-07,
        'enc_db': 3.03e-07,
    },
    'gpu/mlp-h256-pp-hard-E131-T3-table': {
        'x1': 1.39e-06,
        'dz': 4.38e-07,
        'de': 1.41e-06,
        'dbias_cols': 6.31e-07,
        'dbias_tiles': 3.88e-07,
        'a2_grad': 1.42e-06,
        'enc_dwt_ordered': 1.55e-06,
        'enc_db_ordered': 1.53e-06,
        'enc_dwt': 1.55e-06,
        'enc_db': 1.53e-06,
    },
    'gpu/mlp-h256-pp-n3-E1822-T3-two-tiles-a-workgroup': {
        'x1': 1.50e-06,
        'dz': 4.42e-07,
        'de': 1.40e-06,
        'dbias_cols': 4.89e-07,
        'a2_grad': 1.57e-06,
        'enc_dwt_ordered': 2.13e-06,
        'enc_db_ordered': 2.26e-06,
        'enc_dwt': 1.91e-06,
        'enc_db': 2.26e-06,
    },
    'gpu/wgrad-h256-Q100003-row-live': {
        'a2_grad': 2.12e-06,
        'a2_grad_accumulated': 2.12e-06,
    },
}


def check(case, errs):
    """Print every figure (worst |got - ref| / max(1, max |ref|) per quantity), then hold each to its bar from BARS.
    IC3_TANH_ERRORS_OUT=<file>: the figures are appended there as JSON lines as well (how the committed figures were taken)."""
    import json
    import os
    for k in sorted(errs):
        print("tanh-window-h256 %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_TANH_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    assert all(b <= CAP for b in bars.values()), case
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)
