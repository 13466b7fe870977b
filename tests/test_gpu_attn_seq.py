"""The attention kernels over a cache that holds SEVERAL sequences, op by op against the CPU oracle at kernel tolerance (tests/attn_seq_cases.py builds the
cases and the references; tests/test_attn_seq_cpu.py checks on the CPU that every case can tell the right visibility rule from three wrong ones).

  * launch_flash_attn through mi355_op_flash_attn_seq: the matrix-core prompt kernel (tile-wide sequence union, open chunks, the per-sub-tile skip) at every head
    form real models run, the split kernel at 1 / 5 / 31 queries, the f16 parity kernel; n_kv_dev below n_kv_max, positions that do not grow with the cell.
  * one batched single-token step through mi355_op_attn_batch_step in its four launch forms: store inside the attention launch (all chunks / chunk lists),
    small-batch store + attention on the lists, generic store + attention.
  * the single-token forms (attn_out.hip, the single-launch decode attention, NEOX) with other sequences' cells in the cache, with and without chunk lists.

Attention rows are held to 2e-5 * max(1, |ref|.max()) (the bound of test_flash_attn_prefill_matrix_cores and test_attn_step_decode_block; f16 V accumulated in
f32 by the oracle).  Each case prints its worst figure (pytest -s)."""
import numpy as np
import pytest

import attn_seq_cases as ac
import kv_store_cases as kc
import oracle_py as oq
from attn_seq_cases import BASE, TOL
from oracle_py import F16, Q5_K, Q6_K, Q8_0, Q8_K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def worst_rel(got: dict, ref: dict) -> float:
    return max(float(np.abs(got[t] - ref[t]).max()) / max(1.0, float(np.abs(ref[t]).max())) for t in ref)


def run_fa(be, c, inp):
    cell_pos, cell_seq, q_pos, q_seq, q, kcache, vcache = inp
    return be.flash_attn(q, c.H, c.G, c.D, c.tk, kcache, c.tv, vcache, cell_pos, q_pos, c.scale, cell_seq=cell_seq, q_seq=q_seq, n_kv=c.n_kv)


def check_fa(be, c):
    inp = ac.fa_inputs(c)
    out = run_fa(be, c, inp)
    assert np.isfinite(out).all()
    rows = ac.checked_rows(c.T, inp[3])
    ref = ac.fa_reference(c, inp, rows)
    w = worst_rel({t: out[t] for t in rows}, ref)
    print(f"{c.id}: worst {w:.3g} over {len(rows)} rows")
    assert w <= TOL, (c.id, w)


@pytest.mark.parametrize("c", ac.prefill_cases(), ids=lambda c: c.id)
def test_prompt_kernel_several_sequences(be, c):
    splits, pf_splits, takes = be.flash_attn_plan(c.T, c.H, c.G, c.D, c.tk, c.tv, c.n_cells)
    assert takes, "the matrix-core prompt kernel must take this case"
    if c.n_cells == 70:
        assert pf_splits == 1
    else:
        assert (c.n_cells + 31) // 32 >= 16 and pf_splits >= 2, pf_splits
    check_fa(be, c)


@pytest.mark.parametrize("c", [c for c in ac.split_cases() if c.kind == "split"], ids=lambda c: c.id)
def test_split_kernel_several_sequences(be, c):
    splits, _, takes = be.flash_attn_plan(c.T, c.H, c.G, c.D, c.tk, c.tv, c.n_cells)
    assert not takes and splits >= 1
    if c.n_cells == 2100:
        assert splits >= 3                                           # 1024 cells per split at most
    if c.layout == "regions":                                        # whole splits hold only other sequences' cells
        cell_pos, cell_seq, q_pos, q_seq, *_ = ac.fa_inputs(c)
        chunk = min(1024, (-(-c.n_kv // splits) + 31) & ~31)         # attn.hip flash_attn_split_kernel
        vis = ac.visible(cell_pos, cell_seq, c.n_kv, q_pos, q_seq, 0)
        foreign = [sp for sp in range(splits) if sp * chunk < c.n_kv and (cell_pos[sp * chunk:min(c.n_kv, (sp + 1) * chunk)] >= 0).any() and
                   not ((vis >= sp * chunk) & (vis < (sp + 1) * chunk)).any()]
        assert splits >= 2 and foreign, (splits, chunk)
    check_fa(be, c)


def test_f16_parity_kernel_several_sequences(be):
    """fa_v_acc_f16 over a shared prefix, at the caps of test_flash_attn_f16_cache_parity_mode: against the oracle in its STOCK mode, 2e-4 of the largest output,
    a tenth of the parallel kernels' distance, 75 % of the compared elements bit-identical."""
    c = next(c for c in ac.split_cases() if c.kind == "parity")
    inp = ac.fa_inputs(c)
    cell_pos, cell_seq, q_pos, q_seq, q, kcache, vcache = inp
    be.set_option("fa_v_acc_f16", 1)
    try:
        out = run_fa(be, c, inp)
    finally:
        be.set_option("fa_v_acc_f16", -1)
    plain = run_fa(be, c, inp)
    oq.set_fa_v_acc_f32(0)
    worst = worst_plain = 0.0
    same = 0
    for t in range(c.T):
        cells = ac.visible(cell_pos, cell_seq, c.n_kv, q_pos, q_seq, t)
        ref = oq.flash_attn(q[t], c.H, c.G, c.D, F16, kcache, F16, vcache, cells, c.scale)
        den = max(1.0, float(np.abs(ref).max()))
        worst = max(worst, float(np.abs(out[t] - ref).max()) / den)
        worst_plain = max(worst_plain, float(np.abs(plain[t] - ref).max()) / den)
        same += int((out[t].reshape(-1) == ref.reshape(-1)).sum())
    print(f"{c.id}: parity {worst:.3g}, plain {worst_plain:.3g}, identical {same}/{c.T * c.H * c.D}")
    assert worst <= 2e-4 and worst * 10 <= worst_plain, (worst, worst_plain)
    assert same >= 0.75 * c.T * c.H * c.D, same


def test_one_sequence_entry_is_the_sequence_entry_with_defaults(be):
    """mi355_op_flash_attn forwards to mi355_op_flash_attn_seq with masks of 1, sequence 0 and n_kv = n_cells: the same bits, prompt and split kernel."""
    for T in (40, 3):
        c = ac.FaCase("prefill" if T >= 32 else "split", 128, 4, Q8_0, Q8_0, 300, "interleaved", T)
        rng = np.random.default_rng(T)
        cell_pos = np.arange(c.n_cells, dtype=np.int32)
        cell_pos[rng.random(c.n_cells) < 0.1] = -1
        cell_pos[0] = 0
        q_pos = np.sort(rng.integers(0, c.n_cells, T)).astype(np.int32)
        q = rng.standard_normal((T, c.H, c.D)).astype(np.float32)
        kcache, vcache = ac.cache_rows(Q8_0, c.G * c.D, c.n_cells, c.n_cells, "k", False), ac.cache_rows(Q8_0, c.G * c.D, c.n_cells, c.n_cells, "v", True)
        old = be.flash_attn(q, c.H, c.G, c.D, Q8_0, kcache, Q8_0, vcache, cell_pos, q_pos, c.scale)
        new = be.flash_attn(q, c.H, c.G, c.D, Q8_0, kcache, Q8_0, vcache, cell_pos, q_pos, c.scale, cell_seq=np.ones(c.n_cells, np.uint64),
                            q_seq=np.zeros(T, np.int32), n_kv=c.n_cells)
        assert (old.view(np.uint32) == new.view(np.uint32)).all()
    with pytest.raises(Exception, match="q_seq"):
        be.flash_attn(q, c.H, c.G, c.D, Q8_0, kcache, Q8_0, vcache, cell_pos, q_pos, c.scale, q_seq=np.full(T, 64, np.int32))


# ---------------------------------------------------------------- the batched step
def run_step(be, c, inp, mode, want_q8k=True):
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, kc0, vc0, _ = inp
    return be.attn_batch_step(mode, q, k_new, v_new, c.H, c.G, c.D, c.tk, kc0, c.tv, vc0, c.n_kv, cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, BASE, c.n_rot,
                              c.neox, c.scale, want_q8k=want_q8k)


def check_step_result(c, inp, new_rows, res, label):
    """One launch form's outputs against the oracle; returns the worst attention distance."""
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, kc0, vc0, _ = inp
    qr, k_rot, k_ref, v_ref = new_rows
    att, kc1, vc1, blk = res
    assert np.isfinite(att).all()
    rb_k, rb_v = kc0.shape[1], vc0.shape[1]
    kc1, vc1 = kc1.reshape(c.n_cells, rb_k), vc1.reshape(c.n_cells, rb_v)
    others = np.ones(c.n_cells, bool)
    others[tok_cell] = False
    assert (kc1[others] == kc0[others]).all() and (vc1[others] == vc0[others]).all(), f"{label}: a cell outside the step's own was written"
    assert (vc1[tok_cell] == v_ref).all(), f"{label}: V rows"                  # no arithmetic before the V row's quantisation: bit-exact
    worst_k, same, inside = kc.code_distance(c.tk, k_rot, k_ref, kc1[tok_cell])
    assert inside and same >= kc.SAME_SHARE, (label, worst_k, same)
    rows = ac.checked_rows(c.T, tok_seq)
    ref = ac.step_reference(c, inp, qr, kc1, vc1, rows)                        # over the rows the device wrote: what its attention saw
    w = worst_rel({t: att[t] for t in rows}, ref)
    assert w <= TOL, (c.id, label, w)
    if blk is not None:
        for t in rows:
            assert (blk[t] == oq.quantize(Q8_K, att[t])).all(), (label, t)
    return w, worst_k, same


@pytest.mark.parametrize("c", ac.step_cases(), ids=lambda c: c.id)
def test_batched_step_launch_forms(be, c):
    inp = ac.step_inputs(c)
    new_rows = ac.step_new_rows(c, inp)
    res = {m: run_step(be, c, inp, m) for m in c.modes}
    for m in c.modes:
        w, wk, same = check_step_result(c, inp, new_rows, res[m], f"mode {m}")
        print(f"{c.id} mode {m}: attention {w:.3g}, K rows {wk:.3g} steps, {same:.4f} identical")
    for m in c.modes:
        if m in (1, 2):                                                        # the three decode forms agree bit for bit
            for a, b, what in zip(res[0], res[m], ("att", "K cache", "V cache", "Q8_K")):
                assert (a.view(np.uint8) == b.view(np.uint8)).all(), (c.id, m, what)
    for m in set(range(4)) - set(c.modes):                                     # a form without a kernel for the case is refused
        with pytest.raises(Exception, match="no form|no chunk lists"):
            run_step(be, c, inp, m)


def test_batched_step_refuses_what_has_no_kernel(be):
    c = next(c for c in ac.step_cases() if c.T == 5 and c.rope == "norm" and c.tk == Q8_0 and c.tv == Q8_0)
    inp = list(ac.step_inputs(c))
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, kc0, vc0, _ = inp
    T = 65                                                                     # more tokens than a batched step holds
    args65 = (np.zeros((T, c.H * c.D), np.float32), np.zeros((T, c.G * c.D), np.float32), np.zeros((T, c.G * c.D), np.float32))
    with pytest.raises(Exception, match="1 .. 64 tokens"):
        be.attn_batch_step(0, *args65, c.H, c.G, c.D, c.tk, kc0, c.tv, vc0, c.n_kv, cell_pos, cell_seq, np.zeros(T, np.int32), np.arange(T, dtype=np.int32) % 64,
                           np.arange(T, dtype=np.int32), BASE, c.n_rot, False, c.scale)
    twice = tok_seq.copy()
    twice[1] = twice[0]                                                        # two tokens of one sequence: the store-fused launch would race
    for mode in (0, 1):
        with pytest.raises(Exception, match="sequence of its own"):
            be.attn_batch_step(mode, q, k_new, v_new, c.H, c.G, c.D, c.tk, kc0, c.tv, vc0, c.n_kv, cell_pos, cell_seq, tok_pos, twice, tok_cell, BASE, c.n_rot,
                               False, c.scale)


# ---------------------------------------------------------------- single-token forms
def single_reference(H, G, D, tkv, inp, kr, v_row, qr, scale):
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, kc0, vc0 = inp
    kc2, vc2 = kc0.copy(), vc0.copy()
    kc2[tok_cell], vc2[tok_cell] = kr, v_row
    cells = ac.visible(cell_pos, cell_seq, cell_pos.size, [tok_pos], [tok_seq], 0)
    with ac.with_v_acc(tkv):
        return oq.flash_attn(qr, H, G, D, tkv, kc2, tkv, vc2, cells, scale).reshape(-1)


def k_row_ok(tkv, kn, k_row, kr, n):
    dk_ref, dk_got = oq.dequantize(tkv, k_row, n), oq.dequantize(tkv, kr, n)
    step = np.abs(kn) * 2.0 ** -10 if tkv == F16 else np.abs(kn).reshape(-1, 32).max(axis=1).repeat(32) / (127 if tkv == Q8_0 else 8)
    assert (np.abs(dk_ref - dk_got) <= 1.01 * step + 1e-7).all()
    assert (dk_ref == dk_got).mean() >= 0.99


@pytest.mark.parametrize("layout", ["ragged", "shared"])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("tkv", [Q8_0, F16], ids=lambda t: ac.TNAME[t])
@pytest.mark.parametrize("H,G,n_cells,t_o", [(8, 2, 70, Q5_K), (8, 4, 130, Q6_K)])
def test_attn_step_with_other_sequences_in_the_cache(be, H, G, n_cells, t_o, tkv, fused, layout):
    """test_attn_step_decode_block's assertions with two more sequences' cells in the cache, without and with the chunk-list walk (bit-identical)."""
    D = 128
    E = K = H * D
    inp = ac.single_inputs(H, G, n_cells, layout, tkv)
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, kc0, vc0 = inp
    q = q[False]
    rng = np.random.default_rng(H * 1000 + n_cells + t_o)
    W = ac.rand_kquant_weights(rng, t_o, E * K)
    resid = rng.standard_normal(E).astype(np.float32)
    scale = 1 / np.sqrt(D)
    rb = oq.row_bytes(tkv, G * D)
    res = [be.attn_step(q, k_new, v_new, H, G, D, tkv, kc0, tkv, vc0, cell_pos, tok_pos, tok_cell, BASE, D, scale, t_o, W, E, resid, fused, rb, rb,
                        cell_seq=cell_seq, tok_seq=tok_seq, use_lists=ul) for ul in (False, True)]
    for a, b in zip(*res):
        assert (a.view(np.uint8) == b.view(np.uint8)).all(), "with lists != without lists"
    att, out, kr, vr = res[0]
    qr = oq.rope(q, H, D, tok_pos, BASE)
    kn = oq.rope(k_new, G, D, tok_pos, BASE).reshape(-1)
    v_row = oq.quantize(tkv, v_new)
    assert (vr == v_row).all()
    k_row_ok(tkv, kn, oq.quantize(tkv, kn), kr, G * D)
    ref_att = single_reference(H, G, D, tkv, inp, kr, v_row, qr, scale)
    w = float(np.abs(att - ref_att).max()) / max(1.0, float(np.abs(ref_att).max()))
    print(f"attn_step H{H}G{G} c{n_cells} {ac.TNAME[tkv]} fused {fused} {layout}: {w:.3g}")
    assert w <= TOL, w
    ref_out = resid + oq.mul_mat(t_o, W, E, K, att.reshape(1, -1))[0]
    assert np.abs(out - ref_out).max() <= 2e-5 * max(1.0, float(np.abs(ref_out - resid).max())) + 1e-6
    ref_e2e = resid + oq.mul_mat(t_o, W, E, K, ref_att.reshape(1, -1))[0]
    assert np.abs(out - ref_e2e).max() <= 3e-2 * max(1.0, float(np.abs(ref_e2e - resid).max()))


@pytest.mark.parametrize("layout", ["ragged", "shared"])
@pytest.mark.parametrize("tkv", [Q8_0, F16], ids=lambda t: ac.TNAME[t])
@pytest.mark.parametrize("H,G,n_cells", [(8, 2, 70), (8, 4, 130)])
def test_attn_decode_neox_with_other_sequences_in_the_cache(be, H, G, n_cells, tkv, layout):
    D = 128
    inp = ac.single_inputs(H, G, n_cells, layout, tkv)
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, kc0, vc0 = inp
    q = q[True]
    scale = 1 / np.sqrt(D)
    rb = oq.row_bytes(tkv, G * D)
    res = [be.attn_decode_neox(q, k_new, v_new, H, G, D, tkv, kc0, tkv, vc0, cell_pos, tok_pos, tok_cell, BASE, scale, None, None, 0.0, 1, rb, rb,
                               cell_seq=cell_seq, tok_seq=tok_seq, use_lists=ul) for ul in (False, True)]
    for a, b in zip(*res):
        assert (a.view(np.uint8) == b.view(np.uint8)).all(), "with lists != without lists"
    att, kr, vr = res[0]
    qr = oq.rope(q, H, D, tok_pos, BASE, neox=True)
    kn = oq.rope(k_new, G, D, tok_pos, BASE, neox=True).reshape(-1)
    v_row = oq.quantize(tkv, v_new)
    assert (vr == v_row).all()
    k_row_ok(tkv, kn, oq.quantize(tkv, kn), kr, G * D)
    ref_att = single_reference(H, G, D, tkv, inp, kr, v_row, qr, scale)
    w = float(np.abs(att - ref_att).max()) / max(1.0, float(np.abs(ref_att).max()))
    print(f"attn_decode_neox H{H}G{G} c{n_cells} {ac.TNAME[tkv]} {layout}: {w:.3g}")
    assert w <= TOL, w
