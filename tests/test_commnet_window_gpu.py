"""GPU: ic3_commnet_backward (ops.commnet_backward) — the non-recurrent CommNet module's window backward as ONE host call — and its
two new launches alone (ops.commnet_pass_backward, ops.commnet_forward_record) against the float64 window backward of
tests/commnet_window_ref.py on played env states with synthetic weights, masks and head gradients: ragged last tiles, dead and
gated agents in both comm modes, shared weights at hid 256, comm_mask_zero, launches whose workgroups walk more than one tile,
collection-mode masks with two windows accumulated onto the same gradients, a window forced into chunks.  Every entry case is
launched a second time on fresh copies: bit-identical."""
import numpy as np
import pytest
import torch

import commnet_window_ref as ref

pytestmark = pytest.mark.gpu


def _pp(N, dim, vision, E):
    from test_env_parity_gpu import make_pp
    return make_pp(N, dim, vision, 'mixed', E, seed=3)


def _tj(N, dim, difficulty, E):
    from test_env_parity_gpu import make_tj
    return make_tj(N, dim, 1, difficulty, E, seed=3, add_rate_min=0.5, add_rate_max=0.5)


def _record_states(env, T):
    """T snapshots of random play, two steps apart, and the dense observation of each on the CPU in float64"""
    E, N = env.nenvs, env.nagents_env
    rng = np.random.default_rng(7)
    env.reset()
    snaps = torch.empty((T, env.dims.state_words), dtype=torch.int32, device=env.device)
    obs = []
    for t in range(T):
        for _ in range(2):
            env.step(rng.integers(0, env.dims.naction, (E, N)), observe=False)
        env.snapshot(out=snaps[t])
        obs.append(env.observe().reshape(E * N, env.obs_dim).cpu().double().numpy())
    return snaps, obs


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _num(v):
    return v.double().cpu().numpy()


# ---- the pass launch alone ----------------------------------------------------------------------------------------------------
PASS_CASES = [
    # H, Q, OT, dh_in, dhead
    (128, 64 * 3 + 5, 6, False, True),        # the last pass: heads alone, a ragged last tile
    (64, 130, 16, True, False),               # an inner pass
    (256, 64 * 2 + 63, 9, True, True),        # F streamed from L2
    (128, 64 * 300 + 1, 6, True, True),       # 301 tiles on 256 workgroup slots: a workgroup walks two tiles
]


@pytest.mark.parametrize("H,Q,OT,with_dh,with_heads", PASS_CASES)
def test_pass_backward_against_float64(H, Q, OT, with_dh, with_heads):
    """dz (both copies, the same bits), dz . F, dx written and then added to, the partials' column sums written and then added to."""
    from ic3net_amd import ops
    dev = torch.device('cuda')
    rng = np.random.default_rng(H * 7 + Q)
    rn = lambda *s: rng.standard_normal(s)
    h = ref._f32(np.tanh(rn(Q, H)))
    dh_in = ref._f32(rn(Q, H)) if with_dh else None
    dhead, w_heads = (ref._f32(rn(Q, OT)), ref._f32(rn(OT, H) / H ** 0.5)) if with_heads else (None, None)
    fw = ref._f32(rn(H, H) / H ** 0.5)
    v = (dh_in.astype(np.float64) if with_dh else 0.0) + (dhead.astype(np.float64) @ w_heads.astype(np.float64) if with_heads else 0.0)
    want_dz = v * (1.0 - h.astype(np.float64) ** 2)
    want_zf = want_dz @ fw.astype(np.float64)
    nparts = ops.commnet_pass_backward_partials(Q, H)
    tiles = (Q + 63) // 64
    assert nparts < tiles if Q > 64 * 256 else nparts == tiles
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    dxh, dz, dx, parts = nan(Q, 2 * H), nan(Q, H), nan(Q, H), nan(nparts, H)
    args = (_up(dh_in, dev), _up(h, dev), _up(dhead, dev), _up(w_heads, dev), _up(fw, dev), dxh, dz, dx, parts)
    assert ops.commnet_pass_backward(*args) == nparts
    assert torch.equal(dxh[:, :H], dz)
    errs = dict(dz=ref.rel_err(_num(dz), want_dz), dzF=ref.rel_err(_num(dxh[:, H:]), want_zf), dx=ref.rel_err(_num(dx), want_dz),
                bias_cols=ref.rel_err(_num(parts).sum(0), want_dz.sum(0)))
    dx0 = ref._f32(rn(Q, H))
    dx.copy_(_up(dx0, dev))
    assert ops.commnet_pass_backward(*args, dx_add=True, accumulate=True) == nparts
    errs['dx_add'] = ref.rel_err(_num(dx), dx0.astype(np.float64) + want_dz)
    errs['bias_cols_acc'] = ref.rel_err(_num(parts).sum(0), 2 * want_dz.sum(0))
    ref.check("gpu_pass_H%d_Q%d_%s%s" % (H, Q, 'd' if with_dh else '', 'h' if with_heads else ''), errs)


# ---- the recording forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,P,E,N,mode_avg,comm_zero,split", [(128, 2, 131, 3, True, False, True), (64, 3, 130, 5, False, False, False),
                                                             (256, 2, 40, 10, True, True, True)])
def test_forward_record_against_forward_and_float64(H, P, E, N, mode_avg, comm_zero, split):
    """Slot P of the ring is ic3_commnet_forward's h_out, bit for bit (fp32 and split products); every slot against float64; slot 0
    written over enc."""
    from ic3net_amd import ops
    dev = torch.device('cuda')
    rng = np.random.default_rng(H + P + E)
    R, OT = E * N, 6
    w = ref.make_weights(11 + P, H, P, OT, 7)
    cw, fw = [_up(a, dev) for a in w['c_w']], [_up(a, dev) for a in w['f_w']]
    zb = [torch.zeros(H, device=dev)] * P
    wp, _ = ops.commnet_pack(cw, fw, zb, zb)
    wp3 = ops.commnet_pack_split(cw, fw) if split else None
    bias = _up(w['bias'], dev)
    enc = ref._f32(rng.standard_normal((R, H)))
    alive, gate = ref.make_masks(rng, 1, E, N, dead=0.2, gated=0.3)
    al, gt = _up(alive[0], dev), _up(gate[0], dev)
    h0 = torch.full((R, H), float('nan'), device=dev)
    ops.commnet_forward(_up(enc, dev), E, N, wp, bias, _up(w['w_heads'], dev), torch.zeros(OT, device=dev), [OT - 1], mode_avg, comm_zero,
                        al, gt, h_out=h0, wp3=wp3)
    ring = torch.full((P + 1, R, H), float('nan'), device=dev)
    ring[0].copy_(_up(enc, dev))
    ops.commnet_forward_record(ring[0], E, N, wp, bias, mode_avg, comm_zero, al, gt, ring, wp3=wp3)
    torch.cuda.synchronize()
    assert torch.equal(ring[P], h0)
    want = ref.window_backward([enc], None, None, w['f_w'], w['c_w'], w['bias'], w['w_heads'], np.zeros((1, R, OT)), E, N, alive=alive,
                               gate=gate, mode_avg=mode_avg, comm_zero=comm_zero)['h_pass'][:, 0]
    ref.check("gpu_record_H%d_P%d" % (H, P), dict(h_pass=ref.rel_err(_num(ring), want)))


# ---- the whole entry ----------------------------------------------------------------------------------------------------------
ENTRY_CASES = {
    # PP N = 3: 21 envs = 63 rows per communication tile (one idle row); T x R = 1179 rows = 18 tiles + 27 rows; avg mode, gates
    'gpu_entry_pp_n3_E131_T3_h128_P2_avg': dict(env=lambda: _pp(3, 6, 1, 131), H=128, T=3, P=2, mode_avg=True, gates=True),
    # TJ-easy N = 5, sum mode, hard-attention gates with zeros, dead agents
    'gpu_entry_tj_easy_E130_T4_h64_P1_sum': dict(env=lambda: _tj(5, 6, 'easy', 130), H=64, T=4, P=1, mode_avg=False, gates=True, dead=0.3),
    # hid 256 (F streamed from L2, one 512-thread communication workgroup per CU), one F and one C for both passes
    'gpu_entry_pp_hard_E40_T2_h256_P2_share': dict(env=lambda: _pp(10, 20, 1, 40), H=256, T=2, P=2, mode_avg=True, gates=True, share=True),
    # comm_mask_zero: C sees zeros — dh = dz F alone, C's gradient buffers stay as they were
    'gpu_entry_pp_n3_E9_T2_h64_P3_zero': dict(env=lambda: _pp(3, 6, 1, 9), H=64, T=2, P=3, mode_avg=True, gates=False, comm_zero=True),
    # 11400 envs = 543 communication tiles on 512 slots, 34200 rows = 535 row tiles on 256: persistent workgroups walk two tiles
    'gpu_entry_pp_n3_E5700_T2_h128_P1_walk': dict(env=lambda: _pp(3, 6, 1, 5700), H=128, T=2, P=1, mode_avg=True, gates=True, walk=True),
    # collection mode: envs that start an episode inside the window (nobody dead, gated off), two windows of 2 steps onto the same
    # gradients and encoder sums, the later one first; the reference runs over all 4 steps once
    'gpu_entry_tj_easy_E67_T4_h64_P2_collect_two_windows': dict(env=lambda: _tj(5, 6, 'easy', 67), H=64, T=4, P=2, mode_avg=True,
                                                                gates=True, dead=0.3, fresh=0.3, windows=((2, 2), (0, 2))),
    # the first case's window forced into chunks of one step and of two (a short last chunk)
    'gpu_entry_pp_n3_E131_T3_h128_P2_chunk1': dict(env=lambda: _pp(3, 6, 1, 131), H=128, T=3, P=2, mode_avg=True, gates=True, chunk=1),
    'gpu_entry_pp_n3_E131_T3_h128_P2_chunk2': dict(env=lambda: _pp(3, 6, 1, 131), H=128, T=3, P=2, mode_avg=True, gates=True, chunk=2),
}


def _launch(env, w, cfg, snaps, alive, gate, dhead):
    """The case's ic3_commnet_backward call(s) on fresh device copies of the gradients (pre-filled with known values)."""
    from ic3net_amd import ops
    dev = env.device
    H, P, OT, T = w['H'], w['P'], w['OT'], cfg['T']
    E, N = env.nenvs, env.nagents_env
    g = torch.Generator().manual_seed(99)
    pre = lambda *s: torch.randn(s, generator=g)
    host = dict(f_grad=[pre(H, H) for _ in range(P)], c_grad=[pre(H, H) for _ in range(P)], bias_grad=[pre(H) for _ in range(P)],
                heads_w=pre(OT, H), heads_b=pre(OT))
    o = {k: [a.to(dev) for a in v] if isinstance(v, list) else v.to(dev) for k, v in host.items()}
    o['pre'] = {k: [_num(a) for a in v] if isinstance(v, list) else _num(v) for k, v in host.items()}
    cw, fw = [_up(a, dev) for a in w['c_w']], [_up(a, dev) for a in w['f_w']]
    zb = [torch.zeros(H, device=dev)] * P
    wp, _ = ops.commnet_pack(cw, fw, zb, zb)
    wp3 = ops.commnet_pack_split(cw, fw) if cfg.get('split', True) else None
    wt, eb, bias, w_heads = _up(w['enc_wt'], dev), _up(w['enc_bias'], dev), _up(w['bias'], dev), _up(w['w_heads'], dev)
    table = env.encode_table(wt) if cfg.get('table') else None
    al, gt, dh = _up(alive, dev), _up(gate, dev), _up(dhead, dev)
    work = {}
    chunks = 0
    for k, (t0, n) in enumerate(cfg.get('windows', ((0, T),))):
        sl = slice(t0, t0 + n)
        rings, c = ops.commnet_backward(env, n, E, N, H, dh[sl].contiguous(), snaps[sl], al[sl].contiguous(),
                                        None if gt is None else gt[sl].contiguous(), wt, eb, wp, bias, w_heads, fw, cw, o['f_grad'],
                                        o['c_grad'], o['bias_grad'], heads_w_grad=o['heads_w'], heads_b_grad=o['heads_b'], wp3=wp3,
                                        loc_table=table, mode_avg=cfg['mode_avg'], comm_zero=cfg.get('comm_zero', False),
                                        enc_first=(k == 0), enc_window=cfg.get('enc_window', True),
                                        max_chunk_steps=cfg.get('chunk', 0), work=work)
        chunks += c
    torch.cuda.synchronize()
    o.update({k: v.clone() for k, v in rings.items()})
    o['chunks'] = chunks
    return o


@pytest.mark.parametrize("name", list(ENTRY_CASES))
def test_commnet_window_backward_against_float64(name):
    """The rings (a window in one chunk), every per-pass gradient, the heads' and the encoder's gradient (the ordered finish) on top
    of their pre-fills against the float64 window backward, each at its bar; then the same call(s) again on fresh copies: the same
    bits everywhere."""
    from ic3net_amd import ops
    cfg = ENTRY_CASES[name]
    env = cfg['env']()
    T, H, P, OT = cfg['T'], cfg['H'], cfg['P'], 6
    E, N = env.nenvs, env.nagents_env
    R = E * N
    assert ops.commnet_backward_supported(env, H, N)
    if cfg.get('walk'):
        assert ops.comm_backward_partials(T * E, N) < (T * E + 64 // N - 1) // (64 // N)
        assert ops.commnet_pass_backward_partials(T * R, H) < (T * R + 63) // 64
    seed = sum(map(ord, name.replace('_chunk1', '').replace('_chunk2', '')))
    rng = np.random.default_rng(seed)
    w = ref.make_weights(seed, H, P, OT, env.obs_dim, share=cfg.get('share', False))
    alive, gate = ref.make_masks(rng, T, E, N, dead=cfg.get('dead', 0.2), gated=0.3)
    if cfg.get('fresh'):                                        # an env that starts an episode: nobody dead, gated off
        fresh = rng.random((T, E)) < cfg['fresh']
        assert fresh.any() and not fresh.all()
        alive[fresh] = 1
        gate[fresh] = 0
    assert (alive.sum(2) >= 2).all()                            # avg mode divides by n_alive - 1
    if not cfg['gates']:
        gate = None
    dhead = ref._f32(rng.standard_normal((T, R, OT)))
    snaps, obs = _record_states(env, T)
    want = ref.reference_of(w, obs, dhead, E, N, alive=alive, gate=gate, mode_avg=cfg['mode_avg'], comm_zero=cfg.get('comm_zero', False))
    got = _launch(env, w, cfg, snaps, alive, gate, dhead)
    want_chunks = len(cfg.get('windows', (0,))) if not cfg.get('chunk') else (T + cfg['chunk'] - 1) // cfg['chunk']
    assert got['chunks'] == want_chunks
    dwt, db = env.encode_backward_window_finish_ordered(H)
    num = {k: [_num(a) for a in v] if isinstance(v, list) else (_num(v) if torch.is_tensor(v) else v) for k, v in got.items()}
    num['enc_dwt'], num['enc_db'] = _num(dwt), _num(db)
    errs = ref.entry_errors(num, want, T, R)
    if cfg.get('comm_zero'):
        assert all(torch.equal(a.cpu().double(), torch.from_numpy(b)) for a, b in zip(got['c_grad'], got['pre']['c_grad']))
    again = _launch(env, w, cfg, snaps, alive, gate, dhead)
    dwt2, db2 = env.encode_backward_window_finish_ordered(H)
    assert torch.equal(dwt, dwt2) and torch.equal(db, db2)
    for k in ('f_grad', 'c_grad', 'bias_grad'):
        assert all(torch.equal(a, b) for a, b in zip(got[k], again[k])), k
    for k in ('heads_w', 'heads_b', 'h_pass', 'dxh', 'dz', 'dx', 'de', 'dh'):
        assert torch.equal(got[k], again[k]), k
    ref.check(name, errs)
