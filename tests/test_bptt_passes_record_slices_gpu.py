"""GPU: ops.bptt_passes_backward handed slices of a window-long per-pass record — gates[i][t0:t1], hs[i][t0:t1], cs[i][t0:t1] of
(P, T, R, .) arrays: the passes of a chunk are not one block, consecutive passes lie a whole window apart — against the same chunks
copied into contiguous rings (P, Tc, R, .), the way bptt._backward_window_multipass hands them over when it re-evaluates the passes.
Both must give the same dgates, dxh, dh, dc and partials BIT FOR BIT: the call takes one pointer per pass and nothing else may depend
on where a pass's rows lie.  Shape h64-pp-n3-E130-T5-P2-chunk2 (tests/test_bptt_passes_gpu.py): chunks of 2 of 5 steps, last chunk
first, so the last one is short.  (This guards the caller that reads the window launch's record, args.window_record_passes; the
call itself is unchanged.)"""
import pytest
import torch

import bptt_passes_ref as ref

pytestmark = pytest.mark.gpu

OT = 6


def _run(env, w, snaps, layout, chunk):
    from ic3net_amd import ops
    dev = env.device
    T, E, N, H, P = w['T'], w['E'], w['N'], w['H'], w['P']
    R = E * N
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    ups = lambda ms: None if ms is None else [up(m) for m in ms]
    gates, hs, cs = up(w['gates']), up(w['hs']), up(w['cs'])       # (P, T, R, .): the record
    dh, dc = up(w['dh']), up(w['dc'])
    dhead, alive, gate = up(w['dhead']), ups(w['alive']), ups(w['gate'])
    wb3, w_heads = ops.policy_pack_split_bwd(up(w['w_ih']), up(w['w_hh'])), up(w['w_heads'])
    cws = [up(a) for a in w['c_weights']]
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    ring = dict(gates=nan(P, chunk, R, 4 * H), hs=nan(P, chunk, R, H), cs=nan(P, chunk, R, H))
    dxh = nan(P, chunk, R, 2 * H)
    g = torch.Generator().manual_seed(99)
    bias = torch.randn((P, (R + 63) // 64, 4 * H), generator=g).to(dev)
    dcw = torch.randn((P, ops.comm_backward_partials(E, N), H, H), generator=g).to(dev)
    out = dict(dgates=nan(P, T, R, 4 * H), dxh=nan(P, T, R, 2 * H))
    first = True
    for t1 in range(T, 0, -chunk):
        t0 = max(t1 - chunk, 0)
        Tn = t1 - t0
        if layout == 'ring':
            for k, src in (('gates', gates), ('hs', hs), ('cs', cs)):
                ring[k][:, :Tn].copy_(src[:, t0:t1])
            g_p, h_p, c_p = ([ring[k][i, :Tn] for i in range(P)] for k in ('gates', 'hs', 'cs'))
        else:
            g_p, h_p, c_p = ([src[i, t0:t1] for i in range(P)] for src in (gates, hs, cs))
            assert g_p[1].data_ptr() - g_p[0].data_ptr() == T * R * 4 * H * 4 and Tn * R * 4 * H * 4 < T * R * 4 * H * 4
        ops.bptt_passes_backward(env, Tn, E, N, H, g_p, h_p, c_p, dhead[t0:t1], snaps[t0:t1], None if alive is None else alive[t0:t1],
                                 gate[t0:t1], wb3, w_heads, cws, dh, dc, [dxh[i, :Tn] for i in range(P)], [bias[i] for i in range(P)],
                                 [dcw[i] for i in range(P)], detach_gap=2, t_first=t0, enc_first=first)
        first = False
        for i in range(P):
            out['dgates'][i, t0:t1].copy_(g_p[i])
            out['dxh'][i, t0:t1].copy_(dxh[i, :Tn])
    env.encode_backward_window_finish(H)
    torch.cuda.synchronize()
    out.update(dh=dh, dc=dc, bias=bias, dcw=dcw)
    return out


def test_record_slices_give_the_bits_of_the_contiguous_rings():
    from ic3net_amd import ops
    from test_bptt_passes_gpu import _pp, _snapshots
    name = 'h64-pp-n3-E130-T5-P2-chunk2'
    env = _pp(3, 6, 1, 130)
    T, H, P, E, N = 5, 64, 2, env.nenvs, env.nagents_env
    assert ops.bptt_passes_backward_supported(env, H, P)
    w = ref.make_window(sum(map(ord, name)), T, E, N, H, OT, P, alive='first_null')
    snaps, _ = _snapshots(env, T)
    a, b = _run(env, w, snaps, 'ring', 2), _run(env, w, snaps, 'slices', 2)
    for k in ('dgates', 'dxh', 'dh', 'dc', 'bias', 'dcw'):
        x, y = a[k].view(torch.int32), b[k].view(torch.int32)
        assert torch.equal(x, y), "%s: %d words differ" % (k, int((x != y).sum()))
        assert bool(torch.isfinite(a[k]).all()), k
    assert not torch.equal(a['dgates'], torch.from_numpy(w['gates']).to(env.device)), "the backward wrote no dgates"
