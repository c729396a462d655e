"""The float64 references and case tables of tests/policy_ops_ref.py themselves: the cell derivative against float64 autograd
through torch.nn.LSTMCell's formula, the heads against torch.log_softmax, the per-workgroup partial rows against the column sums,
and the cases against what they are there to reach (a grid-stride case does exceed 2048 workgroups, env 0 is all dead, ...)."""
import numpy as np
import pytest
import torch

import policy_ops_ref as ref


@pytest.mark.parametrize("H,R,with_dc", [(4, 5, True), (64, 49, False), (256, 13, True)])
def test_cell_references_match_float64_autograd(H, R, with_dc):
    d = ref.cell_backward_inputs(H, R)
    gates = torch.from_numpy(d['gates']).double().requires_grad_(True)
    c0 = torch.from_numpy(d['c_prev']).double().requires_grad_(True)
    i, f, g, o = gates[:, :H].sigmoid(), gates[:, H:2 * H].sigmoid(), gates[:, 2 * H:3 * H].tanh(), gates[:, 3 * H:].sigmoid()
    c1 = f * c0 + i * g
    h1 = o * c1.tanh()
    h_ref, c_ref = ref.cell_forward(d['gates'], d['c_prev'])
    np.testing.assert_allclose(h_ref, h1.detach().numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(c_ref, c1.detach().numpy(), rtol=0, atol=1e-14)
    loss = (h1 * torch.from_numpy(d['dh']).double()).sum()
    if with_dc:
        loss = loss + (c1 * torch.from_numpy(d['dc']).double()).sum()
    loss.backward()
    dg, dcp = ref.cell_backward(d['gates'], d['c_prev'], d['dh'], d['dc'] if with_dc else None)
    np.testing.assert_allclose(dg, gates.grad.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(dcp, c0.grad.numpy(), rtol=0, atol=1e-13)
    # the lstm cell of torch itself (float64), for the forward
    cell = torch.nn.LSTMCell(H, H).double()
    with torch.no_grad():
        cell.weight_ih.zero_(), cell.weight_hh.zero_(), cell.bias_hh.zero_()
        for r in (0, R - 1):                                  # the bias as the gate pre-activations of one row
            cell.bias_ih.copy_(torch.from_numpy(d['gates'][r]).double())
            h2, c2 = cell(torch.zeros(1, H).double(), (torch.zeros(1, H).double(), torch.from_numpy(d['c_prev'][r:r + 1]).double()))
            np.testing.assert_allclose(h_ref[r], h2[0].numpy(), rtol=0, atol=1e-14)
            np.testing.assert_allclose(c_ref[r], c2[0].numpy(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("sizes", ref.HEADS_SIZES)
@pytest.mark.parametrize("wide", [False, True])
def test_heads_reference_matches_torch_log_softmax(sizes, wide):
    xh, h, W, b = ref.heads_inputs(36, 33, sizes, wide)
    assert np.isnan(xh[:, :36 + ref.PAD]).all() and (xh[:, 36 + ref.PAD:] == h).all()
    out = ref.heads(h, W, b, sizes)
    z = torch.from_numpy(h).double() @ torch.from_numpy(W).double().t() + torch.from_numpy(b).double()
    if wide:                                                  # beyond what exp takes in fp32 without the max subtraction
        assert float(z[:, :sizes[0]].max()) > 89.0 and float(z[:, :sizes[0]].min()) > 0.0
    off = 0
    for A in sizes:
        np.testing.assert_allclose(out[:, off:off + A], torch.log_softmax(z[:, off:off + A], -1).numpy(), rtol=0, atol=1e-12)
        off += A
    np.testing.assert_allclose(out[:, off], z[:, off].numpy(), rtol=0, atol=1e-12)
    assert off + 1 == out.shape[1]


@pytest.mark.parametrize("H,R", ref.cell_backward_cases())
def test_partial_rows_and_the_cases_of_the_cell_backward(H, R):
    RL = 256 // (H // 4)
    nb = ref.cell_backward_blocks(R, H)
    if (H, R) in ref.CELL_BWD_STRIDE:
        blocks = (R + RL - 1) // RL
        assert 2048 < blocks < 2 * 2048 and nb == 2048 and R % RL != 0      # two rows on some lanes, a ragged tail
    else:
        assert nb == (R + RL - 1) // RL <= 4 and (R < RL or R % RL == 1)
    rng = np.random.default_rng(R)
    dg = rng.standard_normal((R, 4 * H))
    pr = ref.partial_rows(dg, R, H, nb)
    assert pr.shape == (nb, 4 * H)
    np.testing.assert_allclose(pr.sum(0), dg.sum(0), rtol=0, atol=1e-10)
    for b in {0, 1 % nb, nb - 1}:                                             # a row, summed the slow way
        rows = [r for r in range(R) if (r // RL) % nb == b]
        np.testing.assert_allclose(pr[b], dg[rows].sum(0), rtol=0, atol=1e-11)
    gates = ref.cell_backward_inputs(H, R)['gates']
    if gates.size > 4000:
        spikes = np.isin(np.abs(gates), (0.0, 30.0, 100.0)).mean()
        assert 0.003 < spikes < 0.03 and (np.abs(gates) == 100.0).any()


def test_case_tables_hold_what_they_promise():
    assert set(H for H, _ in ref.cell_backward_cases()) == {4, 8, 16, 32, 64, 128, 256}
    assert sorted(set(H // 4 for H in ref.FUSED_H)) == [1, 2, 4, 8, 16, 32, 64]            # every template instance
    assert any(sum(s) + 1 > 8 for s in ref.FUSED_SIZES) and any(sum(s) + 1 <= 8 for s in ref.FUSED_SIZES)
    assert max(sum(s) + 1 for s in ref.HEADS_SIZES) == 16 and max(ref.HEADS_H) <= 256
    assert any((H // 4) % 8 for H in ref.HEADS_H) and any(H // 4 < 8 for H in ref.HEADS_H)  # ragged / idle lanes of the row group
    cases = ref.comm_cases()
    ids = [ref.comm_id(c) for c in cases]
    assert len(set(ids)) == len(ids)
    vecN = sorted(set(N for kind, N, H, E, ld in cases if kind == 'vec'))
    assert {1, 2, 16, 17, 32, 33, 64} <= set(vecN)
    for kind, N, H, E, ld in cases:
        vector_path = H % 4 == 0 and ld % 4 == 0 and H // 4 <= 256             # the dispatch rule of the launch
        assert vector_path == (kind == 'vec'), (kind, N, H, E, ld)
        h, alive, gate, wide, scale = ref.comm_inputs(N, H, E)
        assert alive[0].sum() == 0
        if E > 1:
            assert alive[1].sum() == 1
        if E > 2:
            assert alive[2].sum() == min(2, N)
        assert set(np.unique(scale)) <= {0.0, 1.0} and wide.shape == (E, N, 2 * H + ref.PAD)
        if E > 3:
            assert 0 < scale.sum() < scale.size
    assert any(E > 256 // (H // 4) for kind, N, H, E, ld in cases if kind == 'vec' and N == 5)   # more than one workgroup
    wide, dead = ref.sample_inputs(5, 51, 5, zero_prob=True)
    lp = wide[:, :, ref.SAMPLE_COL0:ref.SAMPLE_COL0 + 5]
    assert dead.any() and not dead[:, :, -1].any() and np.isneginf(lp[dead]).all() and np.isfinite(lp[~dead]).all()
    np.testing.assert_allclose(np.exp(lp.astype(np.float64)).sum(-1), 1.0, rtol=0, atol=1e-6)
    for which in ref.REFUSALS:
        H, sizes = ref.refusal_args(which)
        assert (H % 4 != 0) or (H // 4) & (H // 4 - 1) or len(sizes) > 4 or sum(sizes) + 1 > 16, which


def test_comm_reference_is_the_literal_form_and_draw_is_the_oracle():
    from oracle import philox
    h, alive, gate, _, _ = ref.comm_inputs(5, 12, 4)
    out = ref.comm(h, alive, gate, True, True)
    for e in range(4):
        m = (alive[e] * gate[e]).astype(np.float64)
        n_alive = alive[e].sum()
        for j in range(5):
            want = sum(m[i] * m[j] * h[e, i].astype(np.float64) for i in range(5) if i != j) / (n_alive - 1 if n_alive > 1 else 1)
            np.testing.assert_allclose(out[e, j], want, rtol=0, atol=1e-14)
    assert not ref.comm(h, alive, gate, True, False).any()
    x = ref.draws_x24(42, 7000, 3, 9, 2, 6, 5)
    assert x[4, 3] == philox.x24(42, 7004, philox.DOMAIN_SAMPLE, 3, 9, 2 * 5 + 3)
    x = ref.draws_x24(9, 4, np.arange(6), np.arange(6) + 2, 1, 6, 5)
    assert x[5, 1] == philox.x24(9, 9, philox.DOMAIN_SAMPLE, 5, 7, 1 * 5 + 1)
    lp = np.log(np.array([0.25, 0.25, 0.5], np.float32))
    assert [ref.draw(lp, int(u * 2 ** 24)) for u in (0.0, 0.2, 0.3, 0.6, 0.99)] == [0, 0, 1, 2, 2]
