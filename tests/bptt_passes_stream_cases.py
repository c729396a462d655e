"""TEST INFRASTRUCTURE: the cases and the assertions that the host-build test (tests/test_host_bptt_passes_stream_cpu.py) and the GPU
test (tests/test_bptt_passes_stream_gpu.py) of ic3_bptt_backward on an ic3_bptt_passes descriptor WITH row factors share.  A test
brings a backend (how snapshots are taken and how the library is called on its arrays); everything else — the synthetic records,
the cuts, what the caller of the library has to do around the call, the float64 reference and the comparison — is here, once.

What the caller does (bptt._backward_window_multipass does the same on the device):
    pass 0 enters on COPIES of the recorded (h, c) with the starting envs' rows zeroed; the masks are cut for those envs;
    dh is multiplied by keep[T - 1] where it enters the window (dc is the gate launch's, through row_keep);
    the window is walked in chunks of whole steps, last first: row_keep = keep[t0:t1], keep_before = keep[t0 - 1] (None at t0 = 0),
    dh / dc carried from chunk to chunk, the partials added to, the encoder's accumulation started by the first call only.
The reference (bptt_passes_stream_ref.stream_backward) gets the RAW records, masks and cuts and forms all of that itself."""
import numpy as np

import bptt_passes_ref as base
import bptt_passes_stream_ref as ref

OT = 6
f32 = lambda a: np.ascontiguousarray(a, np.float32)

# env: ('pp', N, dim, E) / ('tj', N, dim, E) — R = E * N spans two 64-row tiles with a ragged last one at hid 64
CASES = {
    # product-shaped: env 0 starts at slot 0, env 2 at slot 3 (the first slot of the chunk [3, 5)), env 4 at slot 2; keep = 0 in front
    # of each start; a detach-style zero at the window's last slot (env 5) and one elsewhere (env 7, slot 0 = the border of [1, 3))
    'h64-pp-n10-E9-T5-P2-product': dict(env=('pp', 10, 8, 9), H=64, T=5, P=2, alive='first_null',
                                        cuts=lambda T, E: ref.product_cuts(T, E, [(0, 0), (3, 2), (2, 4)], [(4, 5), (0, 7)])),
    # hid 128 with three passes sharing C, on one tile (the emulated launches of the host build cost seconds per tile at this size):
    # two envs, the factors set by hand so that each moves alone — env 0 starts at slot 2 although keep[1] lets its state through,
    # env 1 is cut behind slot 1 without starting at slot 2; the last slot keeps env 1 only
    'h128-pp-n10-E2-T4-P3-share-independent': dict(env=('pp', 10, 8, 2), H=128, T=4, P=3, share=True,
                                                   cuts=lambda T, E: (np.array([[0, 1], [0, 0], [1, 0], [0, 1]], bool),
                                                                      np.array([[1, 1], [1, 0], [0, 1], [0, 1]], bool))),
    'h64-tj-n5-E13-T4-P2-comm-zero-independent': dict(env=('tj', 5, 6, 13), H=64, T=4, P=2, comm_zero=True, alive='all',
                                                      cuts=lambda T, E: ref.independent_cuts(5, T, E)),
}
CHUNK = 2


def chunks(T, most):
    """[(t0, t1)] last chunk first, as the driver walks a window"""
    return [(max(t1 - most, 0), t1) for t1 in range(T, 0, -most)]


def preconditions(name, fresh, keep, T):
    """A case that cannot tell the factors' slots apart fails here: keep = 0 AND keep = 1 at the window's last slot and on every
    chunk border (the slot in front of a chunk), a starting env at a chunk's first slot, and — product-shaped cases — a start at slot
    0 and one mid-window with keep = 0 exactly in front of it; independent cases — a start whose slot in front keeps, and a cut slot
    whose next slot does not start (each factor moves alone somewhere)."""
    assert (~keep[T - 1]).any() and keep[T - 1].any(), "keep at the window's last slot"
    firsts = [t0 for t0, _ in chunks(T, CHUNK) if t0 > 0]
    assert firsts
    for t0 in firsts:
        assert (~keep[t0 - 1]).any() and keep[t0 - 1].any(), "keep on the border in front of slot %d" % t0
    assert any(fresh[t0].any() for t0 in firsts), "a starting env at a chunk's first slot"
    if 'product' in name:
        assert fresh[0].any() and fresh[1:].any()
        assert all(not keep[t - 1, e] for t, e in zip(*np.nonzero(fresh)) if t > 0)
        assert ((~keep[:-1]) & ~fresh[1:]).any(), "a detach-style zero"
    else:
        assert (fresh[1:] & keep[:-1]).any() and ((~keep[:-1]) & ~fresh[1:]).any()


class Case(object):
    """The arrays of one case: synthetic records (bptt_passes_ref.make_window), cuts, the caller's copies and cut masks."""

    def __init__(self, name):
        cfg = CASES[name]
        self.name, self.cfg = name, cfg
        _, N, _, E = cfg['env']
        self.T, self.H, self.P, self.E, self.N, self.R = cfg['T'], cfg['H'], cfg['P'], E, N, E * N
        self.comm_zero, self.avg = cfg.get('comm_zero', False), cfg.get('avg', True)
        self.w = w = base.make_window(sum(map(ord, name)), self.T, E, N, self.H, OT, self.P, share=cfg.get('share', False),
                                      alive=cfg.get('alive', 'none'))
        self.fresh, self.keep = cfg['cuts'](self.T, E)
        preconditions(name, self.fresh, self.keep, self.T)
        live = f32(1.0 - ref.rows(self.fresh, N))
        self.keep_rows = f32(ref.rows(self.keep, N)[:, :, 0])                               # (T, R)
        # what the caller hands the library: pass 0 on zeroed copies, the other passes' records as they are; cut masks
        self.hs_in = w['hs'].copy()
        self.cs_in = w['cs'].copy()
        self.hs_in[0] *= live
        self.cs_in[0] *= live
        self.alive, self.gate = ref.cut_masks(w['alive'], w['gate'], self.fresh, N)
        self.dh_in = f32(w['dh'] * self.keep_rows[self.T - 1][:, None])                      # dh cut where it enters the window
        rng = np.random.default_rng(99)
        self.tiles = (self.R + 63) // 64
        self.bias0 = f32(rng.standard_normal((self.P, self.tiles, 4 * self.H)))
        self.dW0 = f32(rng.standard_normal((2 * self.H, 4 * self.H)))
        self.rng = rng

    def want(self, obs):
        w = self.w
        return ref.stream_backward(w['gates'], w['hs'], w['cs'], w['hs'][0], w['cs'][0], self.fresh, self.keep, w['dhead'], w['w_heads'],
                                   w['w_ih'], w['w_hh'], w['dh'], w['dc'], self.E, self.N, c_weights=w['c_weights'], alive=w['alive'],
                                   gate=w['gate'], mode_avg=self.avg, comm_zero=self.comm_zero, obs=obs, inp=w['inp'])


def errors(case, got, want):
    """got: float arrays of what one run left — dgates (P, T, R, 4H), dxh (P, T, R, 2H), dh, dc, bias (P, tiles, 4H), dcw (P, slots,
    H, H) with its pre-fill dcw0 (None with comm_zero), enc_dwt, enc_db, dW.  Worst |got - ref| / max(1, max |ref|) per quantity."""
    d = lambda a: np.asarray(a, np.float64)
    errs = dict(dgates=ref.rel_err(d(got['dgates']), want['dgates']), dxh=ref.rel_err(d(got['dxh']), want['dxh']),
                dh=ref.rel_err(d(got['dh']), want['dh']), dc=ref.rel_err(d(got['dc']), want['dc']),
                dbias_rows=ref.rel_err(d(got['bias']), d(case.bias0) + want['dbias_rows']),
                dcb=ref.rel_err((d(got['bias']) - d(case.bias0)).sum(1) @ d(case.w['w_ih']), want['dcb']),
                enc_dwt=ref.rel_err(d(got['enc_dwt']), want['enc_dwt']), enc_db=ref.rel_err(d(got['enc_db']), want['enc_db']),
                dW=ref.rel_err(d(got['dW']), d(case.dW0) + want['dW']))
    if not case.comm_zero:
        errs['dcw'] = ref.rel_err(d(got['dcw']).sum(1), d(got['dcw0']).sum(1) + want['dcw'])
    return errs


def run_and_check(where, name, run):
    """`run(case, most)` -> (got, obs): the backend's run of the case in chunks of at most `most` steps (0: the whole window in one
    call).  Whole and chunked are each held to the float64 whole-window reference at the case's bars, and to each other bit for bit
    in dgates, dh and dc (the same launches on the same operands)."""
    case = Case(name)
    whole, obs = run(case, 0)
    chunked, _ = run(case, CHUNK)
    want = case.want(obs)
    assert np.abs(want['dgates']).max() > 1e-3 and np.abs(want['dh']).max() > 1e-3
    e1, e2 = errors(case, whole, want), errors(case, chunked, want)
    for k in ('dgates', 'dh', 'dc'):
        np.testing.assert_array_equal(whole[k], chunked[k], err_msg=k)
    for k in sorted(e1):
        print("bptt-passes-stream %s/%s %s whole %.3e chunks-of-%d %.3e" % (where, name, k, e1[k], CHUNK, e2[k]))
    ref.check('%s/%s' % (where, name), {k: max(e1[k], e2[k]) for k in e1})     # (one bar per quantity: the worse of the two runs)
