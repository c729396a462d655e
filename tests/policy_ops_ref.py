"""TEST INFRASTRUCTURE: float64 references, case tables and the shared assertions for the launch-chain kernels of
ic3net_amd/csrc/policy_ops.hip (ic3_lstm_cell, ic3_lstm_cell_backward, ic3_policy_heads, ic3_lstm_cell_heads,
ic3_comm_masked_mean[_add], ic3_sample_actions).

The references are written from the formulas of the reference project (torch.nn.LSTMCell's pointwise half, log_softmax per head,
the literal (N, N, H) communication block of oracle.policy_ref, the oracle's inverse-CDF draw), not from the kernels' closed forms.
tests/test_policy_ops_ref_cpu.py holds them to float64 autograd / torch.

A test file supplies a BACKEND: an object that runs one call on numpy inputs and hands numpy outputs back (the host build in
tests/test_host_policy_ops_cpu.py, the ops.* wrappers on the GPU in tests/test_policy_ops_gpu.py); the run_* functions below hold
every assertion, so the two files check the same things under the `host/` and `gpu/` bar keys.  Backend methods:
    cell_backward(gates, c_prev, dh, dc, alias, parts) -> (count, dgates, dc_prev, partials (2048, 4H) NaN-prefilled or None);
                                                     count: the call's return (None where a wrapper tells it only with partials)
    cell_forward(gates, c, H)                     -> (c', xh (R, 2H + 4) NaN-prefilled, h' in its columns [H + 4, 2H + 4))
    heads(xh, H, W, b, sizes)                     -> out (R, OT); h is the column slice xh[:, H + 4:]
    cell_heads(gates, c, H, W, b, sizes, env)     -> (c', xh, out, action (heads, E, N) or None)
    comm(h, H, alive, gate, avg, mask_self, addend, lda_cols, row_scale) -> out (E, N, H); h / addend (E, N, ld) rows: the first H
                                                     columns of each row are the operand, ld its row stride
    sample(wide, col0, A, head, seed, offset, episode, t) -> (action (E, N), chosen log-prob (E, N)); wide (E, N, OT)
    sample_env(env, wide, col0, A, head)          -> action (E, N)
    make_env(E, N)                                -> env with the device counters stepped off zero
    env_counters(env)                             -> (seed, offset, episode (E,), t (E,))
    refusal(which)                                -> runs the named refused call (must raise)

`python tests/policy_ops_ref.py --measure host.jsonl [gpu.jsonl]` turns the figures the tests appended to those files
(IC3_POLICY_OPS_ERRORS_OUT=<file>) into tests/policy_ops_bars.py and profiles/policy_ops_errors.txt."""
import numpy as np

CAP = 1e-5                       # the north-star bound: no bar is above it
MAX_PARTIALS = 2048              # IC3_LSTM_BWD_MAX_PARTIALS
PAD = 4                          # the [x | pad | h] buffers of the cases: row stride 2H + 4, h at column H + 4


# ---- float64 references -------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _split(gates):
    H = gates.shape[1] // 4
    g = np.asarray(gates, np.float64)
    return g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]


def cell_forward(gates, c):
    """torch.nn.LSTMCell's pointwise half, gate order i, f, g, o -> (h', c')."""
    zi, zf, zg, zo = _split(gates)
    i, f, g, o = _sigmoid(zi), _sigmoid(zf), np.tanh(zg), _sigmoid(zo)
    c1 = f * np.asarray(c, np.float64) + i * g
    return o * np.tanh(c1), c1


def cell_backward(gates, c_prev, dh, dc):
    """The derivative of cell_forward by the chain rule, one node at a time: (dL/dh', dL/dc' or None) -> (dL/dgates, dL/dc)."""
    zi, zf, zg, zo = _split(gates)
    c_prev, dh = np.asarray(c_prev, np.float64), np.asarray(dh, np.float64)
    i, f, g, o = _sigmoid(zi), _sigmoid(zf), np.tanh(zg), _sigmoid(zo)
    c1 = f * c_prev + i * g
    t = np.tanh(c1)
    d_o = dh * t                                       # h' = o tanh(c')
    d_c1 = dh * o * (1.0 - t * t)
    if dc is not None:
        d_c1 = d_c1 + np.asarray(dc, np.float64)
    d_f, d_i, d_g = d_c1 * c_prev, d_c1 * g, d_c1 * i  # c' = f c + i g
    dgates = np.concatenate([d_i * i * (1.0 - i), d_f * f * (1.0 - f), d_g * (1.0 - g * g), d_o * o * (1.0 - o)], 1)
    return dgates, d_c1 * f


def partial_rows(dgates, R, H, nblocks):
    """(nblocks, 4H): the float64 sum of dgates over exactly the rows workgroup b walks (row r belongs to (r // RL) % nblocks)."""
    RL = 256 // (H // 4)
    span = RL * nblocks                                # rows of one sweep of the grid
    sweeps = (R + span - 1) // span
    padded = np.zeros((sweeps * span, 4 * H))
    padded[:R] = np.asarray(dgates, np.float64)
    return padded.reshape(sweeps, nblocks, RL, 4 * H).sum((0, 2))


def cell_backward_blocks(R, H):
    RL = 256 // (H // 4)
    return min((R + RL - 1) // RL, MAX_PARTIALS)


def heads(h, W, b, sizes):
    """[log_softmax(W_0 h + b_0) | ... | w_v h + b_v] in float64."""
    z = np.asarray(h, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
    out = z.copy()
    off = 0
    for A in sizes:
        zz = z[:, off:off + A]
        mx = zz.max(1, keepdims=True)
        out[:, off:off + A] = zz - (mx + np.log(np.exp(zz - mx).sum(1, keepdims=True)))
        off += A
    return out


def comm(h, alive, gate, avg, mask_self):
    """The literal (N, N, H) communication block, env by env."""
    from oracle import policy_ref
    E, N, H = h.shape
    out = np.empty((E, N, H))
    for e in range(E):
        out[e] = policy_ref.comm_block(np.asarray(h[e:e + 1], np.float64), None if alive is None else alive[e],
                                       np.ones(N) if gate is None else gate[e], bool(avg), not mask_self, True)[0]
    return out


def draw(logp_row, x24):
    import oracle
    return oracle.sample_one(logp_row, x24)


def draws_x24(seed, offset, episode, t, head, E, N):
    """(E, N) Philox words of (seed, env id, DOMAIN_SAMPLE, episode, t, head * N + n); episode / t scalars or (E,)."""
    from oracle import philox
    e = np.arange(E)[:, None]
    n = np.arange(N)[None, :]
    ep = np.broadcast_to(np.asarray(episode).reshape(-1, 1), (E, 1))
    tt = np.broadcast_to(np.asarray(t).reshape(-1, 1), (E, 1))
    return philox.x24_vec(seed, offset + e, philox.DOMAIN_SAMPLE, ep, tt, head * N + n).astype(np.int64)


# ---- shared assertions ----------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|); inf when anything is not finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float('inf')
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


class Errors(dict):
    def take(self, key, got, ref):
        self[key] = max(self.get(key, 0.0), rel_err(got, ref))


def check(case, errs):
    """Print every figure, then hold each to its bar from policy_ops_bars.BARS (4 x the measured figure, never above 1e-5).
    IC3_POLICY_OPS_ERRORS_OUT=<file>: the figures are appended there as JSON lines as well (how the committed ones were taken)."""
    import json
    import os
    from policy_ops_bars import BARS
    for k in sorted(errs):
        print("policy-ops %s %s %.3e" % (case, k, errs[k]))
    path = os.environ.get('IC3_POLICY_OPS_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, errs=errs)) + "\n")
    bars = BARS.get(case, {})
    bad = {k: (v, bars.get(k)) for k, v in errs.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)


# ---- cell backward ------------------------------------------------------------------------------------------------------------
CELL_BWD_H = (4, 8, 16, 32, 64, 128, 256)
CELL_BWD_STRIDE = ((256, 8205), (128, 16395), (64, 32789))      # ceil(R / RL) > 2048: some workgroups walk two rows a lane


def cell_backward_cases():
    out = []
    for H in CELL_BWD_H:
        RL = 256 // (H // 4)
        out += [(H, 5), (H, 3 * RL + 1)]
    return out + list(CELL_BWD_STRIDE)


def cell_backward_id(c):
    return "cellbwd-H%d-R%d" % c


def spiked(rng, shape):
    """N(0, 1) with about 1 % of the entries from {0, +-30, +-100} (exp2 overflows there)."""
    a = rng.standard_normal(shape)
    hit = rng.random(shape) < 0.01
    a[hit] = rng.choice([0.0, 30.0, -30.0, 100.0, -100.0], size=int(hit.sum()))
    return a.astype(np.float32)


def cell_backward_inputs(H, R):
    rng = np.random.default_rng(1000 * H + R)
    return dict(gates=spiked(rng, (R, 4 * H)), c_prev=rng.standard_normal((R, H)).astype(np.float32),
                dh=rng.standard_normal((R, H)).astype(np.float32), dc=rng.standard_normal((R, H)).astype(np.float32))


def run_cell_backward(be, prefix, H, R):
    d = cell_backward_inputs(H, R)
    nb = cell_backward_blocks(R, H)
    errs = Errors()
    kept = {}
    for mode in ('none', 'separate', 'aliased'):
        if mode != 'aliased':                                         # (aliased: the reference of 'separate')
            ref_dg, ref_dc = cell_backward(d['gates'], d['c_prev'], d['dh'], None if mode == 'none' else d['dc'])
            ref_parts = partial_rows(ref_dg, R, H, nb)
        for parts in (False, True):
            n, dg, dcp, pr = be.cell_backward(d['gates'], d['c_prev'], d['dh'], None if mode == 'none' else d['dc'],
                                              mode == 'aliased', parts)
            assert n == nb or (n is None and not parts), (mode, parts, n, nb)     # (the grid-stride cases: 2048)
            assert np.isfinite(dg).all() and np.isfinite(dcp).all(), (mode, parts)
            errs.take('dgates', dg, ref_dg)
            errs.take('dc_prev', dcp, ref_dc)
            if parts:
                assert np.isnan(pr[nb:]).all(), "a partial row beyond the returned count was written"
                errs.take('partials', pr[:nb], ref_parts)             # every workgroup's own row, not the column total
            kept[mode, parts] = (dg, dcp)
    for parts in (False, True):                                       # aliased and separate dc: bit for bit
        for a, b in zip(kept['aliased', parts], kept['separate', parts]):
            np.testing.assert_array_equal(a, b)
    for mode in ('none', 'separate'):                                 # ... and the partials change nothing else
        for a, b in zip(kept[mode, False], kept[mode, True]):
            np.testing.assert_array_equal(a, b)
    check(prefix + cell_backward_id((H, R)), errs)


# ---- cell forward -------------------------------------------------------------------------------------------------------------
CELL_FWD_H = (4, 12, 64, 100, 256)
CELL_FWD_R = (1, 777)


def cell_forward_inputs(H, R):
    rng = np.random.default_rng(77 * H + R)
    return spiked(rng, (R, 4 * H)), rng.standard_normal((R, H)).astype(np.float32)


def assert_xh_untouched(xh, H):
    assert np.isnan(xh[:, :H + PAD]).all(), "the x half / padding of the [x | h] buffer was written"
    assert np.isfinite(xh[:, H + PAD:]).all()


def run_cell_forward(be, prefix, H):
    errs = Errors()
    for R in CELL_FWD_R:
        gates, c = cell_forward_inputs(H, R)
        ref_h, ref_c = cell_forward(gates, c)
        c1, xh = be.cell_forward(gates, c, H)
        assert xh.shape == (R, 2 * H + PAD)
        assert_xh_untouched(xh, H)
        errs.take('h', xh[:, H + PAD:], ref_h)
        errs.take('c', c1, ref_c)
    check(prefix + "cellfwd-H%d" % H, errs)


# ---- heads --------------------------------------------------------------------------------------------------------------------
HEADS_H = (4, 8, 28, 36, 64, 128, 256)
HEADS_R = (1, 33, 777)
HEADS_SIZES = ([5, 2], [2], [1], [1, 1, 1, 1], [5, 2, 3, 4], [15])


def heads_inputs(H, R, sizes, wide):
    """h in [-1, 1] inside a NaN-filled (R, 2H + 4) buffer; `wide`: W scaled so that the logits of a head spread by about 50, and
    the heads' biases moved by +100 / -120 in turn (log_softmax does not see a shift; exp without the max subtraction overflows at
    88 and is 0 below -104, so that a kernel which skipped the subtraction would give inf / nan here)."""
    OT = sum(sizes) + 1
    rng = np.random.default_rng(31 * H + 7 * R + 1000 * OT + len(sizes) + (5 if wide else 0))
    h = np.tanh(rng.standard_normal((R, H))).astype(np.float32)
    W = (rng.standard_normal((OT, H)) * (0.3 if not wide else 25.0 / np.sqrt(H))).astype(np.float32)
    b = rng.standard_normal(OT).astype(np.float32)
    if wide:
        off = 0
        for k, A in enumerate(sizes):
            b[off:off + A] += -120.0 if k % 2 else 100.0
            off += A
    xh = np.full((R, 2 * H + PAD), np.nan, np.float32)
    xh[:, H + PAD:] = h
    return xh, h, W, b


def run_heads(be, prefix, H):
    errs = Errors()
    spread = 0.0
    for R in HEADS_R:
        for sizes in HEADS_SIZES:
            for wide in ((False, True) if (R == 33) else (False,)):
                xh, h, W, b = heads_inputs(H, R, sizes, wide)
                ref = heads(h, W, b, sizes)
                out = be.heads(xh, H, W, b, sizes)
                assert out.shape == ref.shape
                errs.take('out_spread' if wide else 'out', out, ref)
                if wide and sizes[0] > 1:
                    spread = max(spread, float(-ref[:, :sizes[0]].min()))
    assert spread > 25.0, spread                   # the spread variant does put the log-probs tens of units apart
    check(prefix + "heads-H%d" % H, errs)


# ---- fused cell + heads (+ draws) -----------------------------------------------------------------------------------------------
FUSED_H = (4, 8, 16, 32, 64, 128, 256)
FUSED_SIZES = ([5, 2], [5, 2, 3, 4], [3], [4, 4])  # OT = 8 (the 8-column instance's last), 15 and 9 (the 16-column one), one head
FUSED_EN = ((37, 3), (5, 7))


def fused_inputs(H, E, N, sizes):
    R, OT = E * N, sum(sizes) + 1
    rng = np.random.default_rng(13 * H + R + OT)
    return (spiked(rng, (R, 4 * H)), rng.standard_normal((R, H)).astype(np.float32),
            (rng.standard_normal((OT, H)) * 0.3).astype(np.float32), rng.standard_normal(OT).astype(np.float32))


def check_draws(act, logp, x24, what):
    """Every draw equals the oracle's on the stored log-probabilities; a mismatch only with u within 1e-6 of a cdf edge (expf
    rounding).  Returns the number of such mismatches."""
    act, x24 = act.reshape(-1), x24.reshape(-1)
    logp = logp.reshape(len(act), -1)
    mism = 0
    for r in range(len(act)):
        want = draw(logp[r], int(x24[r]))
        if want != act[r]:
            mism += 1
            u = x24[r] / 2.0 ** 24
            cdf = np.cumsum(np.exp(logp[r].astype(np.float64)))
            assert 0 <= act[r] < logp.shape[1] and np.abs(cdf - u).min() < 1e-6, (what, r, act[r], want)
    return mism


def run_fused(be, prefix, H):
    errs = Errors()
    mism = ndraws = 0
    for E, N in FUSED_EN:
        env = be.make_env(E, N)
        seed, offset, episode, t = be.env_counters(env)
        assert (np.asarray(t) > 0).any()                                  # the counters are off zero
        for sizes in FUSED_SIZES:
            gates, c, W, b = fused_inputs(H, E, N, sizes)
            R, OT = E * N, sum(sizes) + 1
            ref_h, ref_c = cell_forward(gates, c)
            c_u, xh_u = be.cell_forward(gates, c, H)                      # the unfused launch
            c_f, xh_f, out_f, act = be.cell_heads(gates, c, H, W, b, sizes, env)
            np.testing.assert_array_equal(c_f, c_u)                       # cell outputs: bit for bit the unfused kernel's
            np.testing.assert_array_equal(xh_f, xh_u)
            assert_xh_untouched(xh_f, H)
            errs.take('h', xh_f[:, H + PAD:], ref_h)
            errs.take('c', c_f, ref_c)
            # the heads against float64 on the kernel's own stored h (what policy_heads would read) — not against policy_heads
            errs.take('out', out_f, heads(xh_f[:, H + PAD:], W, b, sizes))
            errs.take('out_end_to_end', out_f, heads(ref_h, W, b, sizes))
            assert act.shape == (len(sizes), E, N)
            wide = out_f.reshape(E, N, OT)
            off = 0
            for k, A in enumerate(sizes):
                np.testing.assert_array_equal(act[k], be.sample_env(env, wide, off, A, k))
                mism += check_draws(act[k], wide[:, :, off:off + A], draws_x24(seed, offset, episode, t, k, E, N),
                                    (H, E, N, sizes, k))
                ndraws += E * N
                off += A
            c_n, xh_n, out_n, act_n = be.cell_heads(gates, c, H, W, b, sizes, None)     # no env handle: no draws, same outputs
            assert act_n is None
            np.testing.assert_array_equal(out_n, out_f)
            np.testing.assert_array_equal(c_n, c_f)
            np.testing.assert_array_equal(xh_n, xh_f)
    print("policy-ops %sfused-H%d draws %d cdf-edge mismatches %d" % (prefix, H, ndraws, mism))
    assert mism <= 2 * ((ndraws + 5119) // 5120)
    check(prefix + "fused-H%d" % H, errs)


# ---- communication block ------------------------------------------------------------------------------------------------------
def comm_cases():
    """(kind, N, H, E, ldh): 'vec' the float4 instances (N <= 16, N <= 32, the two-pass loop), 'scalar' the fallback."""
    out = [('vec', N, 64, 9, 64) for N in (1, 2, 16, 17, 32, 33, 64)]
    for H in (4, 12, 300, 384, 1024):
        out += [('vec', 5, H, 1, H), ('vec', 5, H, 256 // (H // 4) + 1, H)]
    out += [('scalar', N, H, 3, H) for H in (6, 30, 1028) for N in (3, 40)]
    out.append(('scalar', 5, 64, 4, 2 * 64 + 2))
    return out


def comm_id(c):
    return "comm-%s-N%d-H%d-E%d%s" % (c[0], c[1], c[2], c[3], "" if c[4] == c[2] else "-ld%d" % c[4])


def comm_inputs(N, H, E):
    """h, masks (env 0 all dead, env 1 one agent alive, env 2 two alive), an addend inside a wider buffer, a 0 / 1 row scale."""
    rng = np.random.default_rng(100000 * N + 10 * H + E)
    h = rng.standard_normal((E, N, H)).astype(np.float32)
    alive = (rng.random((E, N)) < 0.7).astype(np.int32)
    gate = (rng.random((E, N)) < 0.6).astype(np.int32)
    for e in range(min(E, 3)):
        alive[e] = 0
        alive[e, rng.permutation(N)[:min(e, N)]] = 1
    wide = rng.standard_normal((E, N, 2 * H + PAD)).astype(np.float32)
    scale = (rng.random((E, N)) < 0.6).astype(np.float32)
    return h, alive, gate, wide, scale


def strided(a, ld):
    """`a` (E, N, H) as the leading columns of a NaN-padded (E, N, ld) buffer."""
    if ld == a.shape[2]:
        return a
    out = np.full(a.shape[:2] + (ld,), np.nan, np.float32)
    out[:, :, :a.shape[2]] = a
    return out


def run_comm(be, prefix, case):
    kind, N, H, E, ldh = case
    h, alive, gate, wide, scale = comm_inputs(N, H, E)
    hs = strided(h, ldh)
    errs = Errors()
    refs = {}
    for avg in (True, False):
        for ua, ug in ((False, False), (True, False), (False, True), (True, True)):
            al, ga = alive if ua else None, gate if ug else None
            refs[avg, ua, ug] = ref = comm(h, al, ga, avg, True)
            errs.take('out', be.comm(hs, H, al, ga, avg, True, None, 0, None), ref)
    z = be.comm(hs, H, alive, gate, True, False, None, 0, None)          # comm_mask_zero
    assert z.shape == (E, N, H) and not z.any()
    if kind == 'scalar':
        import pytest
        with pytest.raises(NotImplementedError, match="multiples of 4"):    # the library's -38
            be.comm(hs, H, alive, gate, True, True, wide, H + PAD, None)
        check(prefix + comm_id(case), errs)
        return
    h2 = strided(h, 2 * H + PAD)                                         # h as the column slice of an [x | h] buffer
    add = wide[:, :, H + PAD:]                                           # the addend as one (row stride 2H + 4)
    a64, s64 = add.astype(np.float64), scale.astype(np.float64)[:, :, None]
    for (avg, ua, ug), ref in refs.items():
        if ua != ug and not avg:
            continue                                                     # (every mask pair in avg mode, none / both in sum mode)
        al, ga = alive if ua else None, gate if ug else None
        errs.take('strided', be.comm(h2, H, al, ga, avg, True, None, 0, None), ref)
        errs.take('addend', be.comm(h2, H, al, ga, avg, True, wide, H + PAD, None), a64 + ref)
        errs.take('row_scale', be.comm(hs, H, al, ga, avg, True, wide, H + PAD, scale), (a64 + ref) * s64)
    errs.take('addend_alone', be.comm(hs, H, alive, gate, True, False, wide, H + PAD, None), a64)
    errs.take('addend_alone_scaled', be.comm(hs, H, alive, gate, True, False, wide, H + PAD, scale), a64 * s64)
    check(prefix + comm_id(case), errs)


# ---- sampling -----------------------------------------------------------------------------------------------------------------
SAMPLE_A = (1, 2, 5, 15)
SAMPLE_EN = ((1, 1), (51, 5), (512, 10))
SAMPLE_HEADS = (0, 2)
SAMPLE_COL0 = 3                                    # the head's first column inside the (E, N, OT) rows
SAMPLE_SEED, SAMPLE_OFFSET, SAMPLE_EPISODE, SAMPLE_T = 42, 7000, 3, 9


def sample_inputs(A, E, N, zero_prob=False):
    """(E, N, OT) rows [3 columns of another head | this head's log-probs | a value column]; zero_prob: in every third row two
    actions (never the last) have probability exactly 0."""
    rng = np.random.default_rng(17 * A + E + N + (1 if zero_prob else 0))
    OT = SAMPLE_COL0 + A + 1
    wide = rng.standard_normal((E, N, OT)).astype(np.float32)
    z = rng.standard_normal((E, N, A)) * 1.5
    dead = np.zeros((E, N, A), bool)
    if zero_prob:
        assert A >= 4
        dead.reshape(-1, A)[::3, 0] = True
        dead.reshape(-1, A)[::3, 2] = True
        z[dead] = -np.inf
    mx = z.max(-1, keepdims=True)
    wide[:, :, SAMPLE_COL0:SAMPLE_COL0 + A] = (z - (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True)))).astype(np.float32)
    return wide, dead


def run_sample(be, A, E, N, zero_prob=False):
    """-> (draws, cdf-edge mismatches) over both head indices."""
    wide, dead = sample_inputs(A, E, N, zero_prob)
    lp = wide[:, :, SAMPLE_COL0:SAMPLE_COL0 + A]
    assert (np.isneginf(lp) == dead).all()
    mism = 0
    for head in SAMPLE_HEADS:
        act, chosen = be.sample(wide, SAMPLE_COL0, A, head, SAMPLE_SEED, SAMPLE_OFFSET, SAMPLE_EPISODE, SAMPLE_T)
        assert act.shape == (E, N) and act.min() >= 0 and act.max() < A
        x = draws_x24(SAMPLE_SEED, SAMPLE_OFFSET, SAMPLE_EPISODE, SAMPLE_T, head, E, N)
        m = check_draws(act, lp, x, (A, E, N, head))
        assert m <= 2 * ((E * N + 5119) // 5120), m
        mism += m
        picked = np.take_along_axis(lp, act[:, :, None].astype(np.int64), 2)[:, :, 0]
        assert chosen.dtype == np.float32 and (chosen.view(np.uint32) == picked.view(np.uint32)).all()   # bit for bit
        assert not np.take_along_axis(dead, act[:, :, None].astype(np.int64), 2).any(), "an action of probability 0 was drawn"
    print("policy-ops sample A%d E%d N%d%s draws %d cdf-edge mismatches %d"
          % (A, E, N, "-zero-prob" if zero_prob else "", 2 * E * N, mism))
    return 2 * E * N, mism


# ---- refusals -----------------------------------------------------------------------------------------------------------------
REFUSALS = {                                       # name -> the exception the library's code maps to (-22 / -38)
    'cell_backward-H6': ValueError, 'cell_backward-H12': NotImplementedError,
    'cell_heads-H6': ValueError, 'cell_heads-H12': NotImplementedError,
    'cell_heads-five-heads': ValueError, 'cell_heads-OT17': ValueError,
    'heads-five-heads': ValueError, 'heads-OT17': ValueError,
}


def refusal_args(which):
    """(H, sizes) of a refused call; R = 3 and every buffer has its full size, so even a launch would stay inside them."""
    H = {'H6': 6, 'H12': 12}.get(which.split('-', 1)[1], 16)
    sizes = [1, 1, 1, 1, 1] if which.endswith('five-heads') else [15, 1] if which.endswith('OT17') else [2]
    return H, sizes


def run_refusal(be, which):
    import pytest
    with pytest.raises(REFUSALS[which]):
        be.refusal(which)


# ---- the figures -> bars ------------------------------------------------------------------------------------------------------
def _measure(paths):
    import json
    import os
    fig = {}
    for path in paths:
        for line in open(path):
            rec = json.loads(line)
            for k, v in rec['errs'].items():
                d = fig.setdefault(rec['case'], {})
                d[k] = max(d.get(k, 0.0), v)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows, bars = [], {}
    host = sorted(c for c in fig if c.startswith('host/'))
    for hc in host:
        for case in (hc, 'gpu/' + hc[5:]):
            for k in fig[hc]:
                v = fig.get(case, {}).get(k)
                bar = CAP if v is None else min(CAP, 4.0 * v)
                bars.setdefault(case, {})[k] = bar
                rows.append("%-36s %-20s %-10s %.2e" % (case, k, "-" if v is None else "%.2e" % v, bar))
    # both files keep their hand-written text: the comment lines in front of the rows (and from "# ----" on behind them), the
    # docstring in front of BARS
    path = os.path.join(root, 'profiles', 'policy_ops_errors.txt')
    old = open(path).read().split("\n") if os.path.exists(path) else []
    head = old[:next((i for i, s in enumerate(old) if not s.startswith('#')), len(old))]
    tail = old[next((i for i, s in enumerate(old) if s.startswith('# ----')), len(old)):]
    with open(path, 'w') as f:
        f.write("\n".join(head + rows + ([""] + tail if tail else [])).rstrip("\n") + "\n")
    path = os.path.join(root, 'tests', 'policy_ops_bars.py')
    text = open(path).read()
    with open(path, 'w') as f:
        f.write(text[:text.index("BARS = {")] + "BARS = {\n")
        for case in bars:
            f.write("    %r: {\n" % case)
            for k, b in bars[case].items():
                f.write("        %r: %.2e,\n" % (k, b))
            f.write("    },\n")
        f.write("}\n")
    worst = max((v, c, k) for c in fig for k, v in fig[c].items())
    print("worst figure %.3e (%s %s); %d rows" % (worst + (len(rows),)))


if __name__ == "__main__":
    import sys
    assert len(sys.argv) >= 3 and sys.argv[1] == "--measure", __doc__
    _measure(sys.argv[2:])
