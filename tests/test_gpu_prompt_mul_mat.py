"""The dense prompt batch's mat-mul launches, op by op: every launch of tests/prompt_mul_mat_cases.py through Backend.prompt_mul_mat - the launchers the model
issues it with - against the oracle within the project's bound, on the path the case names, with the whole padded out buffers checked: nothing unwritten or
NaN inside N (the buffers are 0xFF bytes before the launch), the pad columns still 0xFF.  Then the relations the kernels' code states, bit for bit: the residual
epilogue = resid + the stored result; in place = out of place; a segment of a several-segment launch = the tensor launched alone; a producer that writes the
bh / bl planes itself = the quantiser followed by launch_mmq_prep.  Then the producers of those planes on their own (Backend.act_q8k_planes, the attention merge)."""
import numpy as np
import pytest

import attn_seq_cases as ac
import np_twin as tw
import oracle_py as oq
import prompt_mul_mat_cases as pc
from attn_seq_cases import BASE
from oracle_py import Q8_K
from prompt_mul_mat_cases import ADD, RUN_CASES, STORE

pytestmark = pytest.mark.gpu

_REF, _INP = {}, {}


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def inputs(c):
    if c["name"] not in _INP:
        _INP[c["name"]] = pc.inputs(c)
    return _INP[c["name"]]


def reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = pc.reference(c, inputs(c))
        for r in _REF[c["name"]]:
            r.setflags(write=False)
    return _REF[c["name"]]


def run(be, c, epi=None, in_place=False, prologue=None, segs=None, form=None, split=None, check=True):
    """The case's launch under its options; segs: only these tensors (a segment on its own); the options go back to their defaults whatever happens."""
    inp = inputs(c)
    epi = c["epi"] if epi is None else epi
    prologue = c["prologue"] if prologue is None else prologue
    segs = range(len(c["types"])) if segs is None else segs
    x = inp["x"] if prologue == c["prologue"] else pc.activation(c, inp)
    be.set_option("mmq_tiles", c["tiles"])
    be.set_option("mmq_split", c["split"] if split is None else split)
    try:
        return be.prompt_mul_mat([c["types"][s] for s in segs], [inp["W"][s] for s in segs], [c["Ns"][s] for s in segs], c["K"], x, epi=epi,
                                 resid=inp["resid"] if epi == ADD else None, in_place=in_place, prologue=prologue, norm_w=inp["nw"] if prologue == 1 else None,
                                 eps=pc.EPS, form=c["form"] if form is None else form, ld_pad=c["ld_pad"], check=check)
    finally:
        be.set_option("mmq_tiles", 0)
        be.set_option("mmq_split", 0)


def check_buffers(c, ys, refs, what="", bound=None):
    """Every out buffer whole: values inside N finite and within the bound of the oracle, the pad columns untouched."""
    assert len(ys) == len(refs)
    for s, (y, ref) in enumerate(zip(ys, refs)):
        N = ref.shape[1]
        assert y.shape == (ref.shape[0], N + c["ld_pad"]), (c["name"], what, s)
        inside = y[:, :N]
        bad = np.argwhere(~np.isfinite(inside))
        assert bad.size == 0, f"{c['name']} {what} segment {s}: unwritten / non-finite results at (token, row) {bad[:8].tolist()} of {len(bad)}"
        assert (y[:, N:].view(np.uint32) == 0xFFFFFFFF).all(), f"{c['name']} {what} segment {s}: a pad column was written"
        err = np.abs(inside - ref)
        i = np.unravel_index(int(err.argmax()), err.shape)
        b = pc.bound(c, ref) if bound is None else bound * float(np.abs(ref).max()) + 1e-6
        print(f"{c['name']} {what} segment {s}: max |err| {err.max():.3e} at {i}, bound {b:.3e}")
        assert err.max() <= b, f"{c['name']} {what} segment {s}: |err| {err.max():.3e} at {i} (got {inside[i]!r}, want {ref[i]!r}) > {b:.3e}"


@pytest.mark.parametrize("c", RUN_CASES, ids=lambda c: c["name"])
def test_launch_matches_oracle_on_its_path(be, c):
    ys, path, _ = run(be, c)
    assert path == c["path"], f"{c['name']}: took {path}"
    check_buffers(c, ys, reference(c))


ADD_CASES = [c for c in RUN_CASES if c["epi"] == ADD]


@pytest.mark.parametrize("c", ADD_CASES, ids=lambda c: c["name"])
def test_add_is_resid_plus_store_in_place_or_not(be, c):
    """Every launcher's residual epilogue is out = resid + v, one IEEE f32 add behind the full sum v that the same launch stores without a residual (mmq.hip:
    mmq_ksplit_kernel, mmq_planes_kernel, planes2_body, mmq_splitk_reduce_kernel, mmq_kernel); and the model runs it with the residual buffer as the out
    buffer, where every element is read by the thread that writes it."""
    ya, pa, _ = run(be, c)
    yi, pi, _ = run(be, c, in_place=True)
    ystore, ps, _ = run(be, c, epi=STORE)
    assert pa == pi == ps == c["path"], (pa, pi, ps)
    N = c["Ns"][0]
    resid = inputs(c)["resid"]
    check_buffers(c, ystore, pc.reference(dict(c, epi=STORE), inputs(c)), "store")
    want = (np.float32(resid[:, :N]) + ystore[0][:, :N]).astype(np.float32)
    assert np.array_equal(ya[0][:, :N], want), c["name"]
    # in place the buffer held the residual's whole rows: inside N the bits of the launch out of place, the pad columns still the residual's
    assert np.array_equal(yi[0][:, :N].view(np.uint32), ya[0][:, :N].view(np.uint32)), c["name"]
    assert np.array_equal(yi[0][:, N:].view(np.uint32), resid[:, N:].view(np.uint32)), f"{c['name']} in place: a pad column was written"


def alone_form(c, path):
    return c["form"] if c["form"] != pc.FORM_MODEL else {1: pc.FORM_KSPLIT, 5: pc.FORM_FLY}.get(path["kernel"], pc.FORM_PLANES)


MULTI_CASES = [c for c in RUN_CASES if len(c["types"]) > 1 and c["epi"] == STORE]


@pytest.mark.parametrize("c", MULTI_CASES, ids=lambda c: c["name"])
def test_segment_is_the_tensor_launched_alone(be, c):
    """A several-segment launch routes tiles to segments (tile0, row_end, out - row_end, ld per segment, mins_mask per row tile) and changes no arithmetic:
    under the same forced tile form and K split every segment has the bits of its tensor launched alone."""
    ys, path, _ = run(be, c)
    for s in range(len(c["types"])):
        y1, p1, _ = run(be, c, segs=[s], form=alone_form(c, path))
        assert (p1["kernel"], p1["n_split"]) == (path["kernel"], path["n_split"]) and not p1["mixed"], (c["name"], s, p1)
        assert np.array_equal(ys[s].view(np.uint32), y1[0].view(np.uint32)), (c["name"], s)


@pytest.mark.parametrize("c", [c for c in RUN_CASES if c["form"] == pc.FORM_MODEL], ids=lambda c: c["name"])
def test_model_choice_is_the_named_launcher(be, c):
    """Form 0 asks host/runtime.cc prompt_mul_mat_choice, as Context::linear, linear_multi and the gate | up block do, and then issues the launcher's own call:
    the bits of the same launch asked for by name.  (The Q | K pair of model_qkv_q6k_alone_t260 fuses and V follows alone: every segment is checked above.)"""
    ys, path, _ = run(be, c)
    if c["name"] == "model_qkv_q6k_alone_t260":
        with pytest.raises(Exception, match="refuses these segments"):     # by name it is one mixed launch, which the 256 x 32 tiles do not take
            run(be, c, form=pc.FORM_PLANES)
        return
    yn, pn, _ = run(be, c, form=alone_form(c, path), in_place=c["epi"] == ADD)
    assert pn == path
    for s, (a, b) in enumerate(zip(ys, yn)):                    # (the named launch of a residual case runs in place: its pad columns hold the residual's)
        N = c["Ns"][s]
        assert np.array_equal(a[:, :N].view(np.uint32), b[:, :N].view(np.uint32)), c["name"]


@pytest.mark.parametrize("c", [c for c in RUN_CASES if c["prologue"] != 0], ids=lambda c: c["name"])
def test_producer_planes_are_the_prep_launch(be, c):
    """The producers write bsum = 64 * bh + bl with mmq_prep_kernel's split (act.hip), and their Q8_K blocks are those of the quantiser's launch over the same
    f32 rows.  Prologue 3 against prologue 0 on the same x: the same bits.  Prologues 1 and 2 against prologue 0 over the oracle's activation rows: the same
    bits where the device's rows are the oracle's, which is printed.  Where its sum of squares or its expf differs in the last place, codes_stable() keeps the
    codes in place and only a block's f32 scale moves by an ulp (6e-8 of its terms): the two results are then held to 2e-6 of the output scale, the project's
    bound for two launches that differ in f32 rounding alone (pc.SPLIT_BOUND)."""
    y, path, _ = run(be, c)
    y0, p0, _ = run(be, c, prologue=0)
    assert path["prep"] == 0 and p0["prep"] == 1 and p0["kernel"] == path["kernel"]
    check_buffers(c, y0, reference(c), "prologue 0")
    if c["prologue"] == 3:
        assert np.array_equal(y[0].view(np.uint32), y0[0].view(np.uint32)), c["name"]
    else:
        same = np.array_equal(y[0].view(np.uint32), y0[0].view(np.uint32))
        print(f"{c['name']}: bit-equal to the quantiser + prep over the oracle's rows: {same}")
        ref = reference(c)[0]
        N = ref.shape[1]
        assert np.abs(y[0][:, :N] - y0[0][:, :N]).max() <= pc.SPLIT_BOUND * float(np.abs(ref).max()) + 1e-6, c["name"]


SPLIT_CASES = [c for c in RUN_CASES if c["path"] and c["path"]["n_split"] > 1]


@pytest.mark.parametrize("c", SPLIT_CASES, ids=lambda c: c["name"])
def test_k_split_against_the_unsplit_launch(be, c):
    """The partial sums of 2 .. 4 K ranges added in split order against the one running sum: 2e-6 of the output scale (test_mul_mat_prefill_split_k)."""
    ys, _, _ = run(be, c)
    yu, pu, _ = run(be, c, split=1)
    assert pu["n_split"] == 1 and pu["kernel"] == pc.KERNEL_LDS
    check_buffers(c, yu, reference(c), "unsplit")
    for s, (a, b) in enumerate(zip(ys, yu)):
        N = c["Ns"][s]
        ref = reference(c)[s]
        d = np.abs(a[:, :N] - b[:, :N]).max()
        print(f"{c['name']} segment {s}: split against unsplit {d:.3e}")
        assert d <= pc.SPLIT_BOUND * float(np.abs(ref).max()) + 1e-6, (c["name"], s, d)


@pytest.mark.parametrize("c", pc.REFUSED_CASES, ids=lambda c: c["name"])
def test_refused_launch_leaves_the_buffers_untouched(be, c):
    ys, path, rc = run(be, c, check=False)
    assert rc == pc.ERR_ARG, (c["name"], rc)
    assert all(v == 0 for v in path.values()), path
    for y in ys:
        assert (y.view(np.uint32) == 0xFFFFFFFF).all(), c["name"]


def test_argument_errors(be):
    c = pc.BY_NAME["add_ksplit_q4k_k512_n37_t5"]
    inp = inputs(c)
    for kw in (dict(epi=ADD, resid=None), dict(epi=STORE, resid=inp["resid"]), dict(epi=STORE, in_place=True), dict(form=4), dict(prologue=1), dict(form=pc.FORM_FLY),
               dict(form=pc.FORM_PLANES)):                        # (the last two: 5 tokens are no prompt batch)
        args = dict(epi=ADD, resid=inp["resid"], form=pc.FORM_KSPLIT, ld_pad=3, check=False)
        args.update(kw)
        ys, path, rc = be.prompt_mul_mat(c["types"], inp["W"], c["Ns"], c["K"], inp["x"], **args)
        assert rc == pc.ERR_ARG, kw
        assert (ys[0].view(np.uint32) == 0xFFFFFFFF).all(), kw


# ---------------------------------------------------------------- the producers of the activation on their own
def check_planes(blk, bh, bl, n, what):
    """bsum = 64 * bh + bl with 0 <= bl <= 63 against the blocks' own block sums: every entry of both planes is accounted for (none left 0xFF unless -1 is the value)."""
    b = np.ascontiguousarray(blk).view(tw.DT[Q8_K])
    bsums = b["bsums"].reshape(blk.shape[0], n // 16).astype(np.int32)
    assert bh.shape == bl.shape == bsums.shape, what
    assert (bl >= 0).all() and (bl <= 63).all(), what
    assert np.array_equal(64 * bh.astype(np.int32) + bl.astype(np.int32), bsums), what
    assert np.array_equal(bh.astype(np.int32), bsums >> 6), what
    return bsums


@pytest.mark.parametrize("n", pc.PRODUCER_N)
@pytest.mark.parametrize("T", pc.PRODUCER_T)
@pytest.mark.parametrize("producer", [0, 1, 2])
def test_producer_blocks_and_planes(be, producer, T, n):
    """launch_quantize, launch_rmsnorm_quant and launch_swiglu_quant as the model calls them before a K-quant layer: Q8_K with bh / bl.  T reaches the narrow
    kernel's split rule (T < 8, T < 64) and the wide kernel (T >= 32); n one and two blocks per wave of it, the two widths where the norm refuses it
    (4352, 5632: n % 1024 != 0; 8448: more than 32 blocks) and the un-normed wide grid of two parts (n > 4096)."""
    x, x2, nw, n_edge = pc.producer_inputs(producer, T, n)
    blk, bh, bl, ph, pl, yf = be.act_q8k_planes(producer, x, x2, nw, pc.EPS, want_f32=producer == 1)
    rows = pc.producer_reference(producer, x, x2, nw)
    bsums = check_planes(blk, bh, bl, n, (producer, T, n))
    assert np.array_equal(bh, ph) and np.array_equal(bl, pl), (producer, T, n)
    for t in range(T):
        assert np.array_equal(blk[t], oq.quantize(Q8_K, rows[t])), (producer, T, n, t)
    for e in range(n_edge):
        bsum, h, l = pc.EDGE_SUMS[e]
        r = T - n_edge + e
        sub = np.arange(n // 16) % 16 != 0
        assert (bsums[r][sub] == bsum).all() and (bh[r][sub] == h).all() and (bl[r][sub] == l).all(), (producer, T, n, e)
    if yf is not None:
        d = np.abs(yf - rows).max() / max(1.0, float(np.abs(rows).max()))
        assert d <= 1e-6, d


@pytest.mark.parametrize("T,n", [(7, 1024), (31, 5120), (40, 8448)])
def test_swiglu_quant_is_swiglu_then_quantise(be, T, n):
    """General gate values, where silu goes through expf: act.hip states that swiglu_quant_kernel has the arithmetic of swiglu_kernel followed by the quantiser.
    The device's own SwiGLU rows are within 2e-5 of the oracle's silu(g) * u (the device's expf and the host's differ in the last place of some values, which
    is why the byte comparison against the oracle above runs on gate values where silu(g) = g); the blocks are the oracle's quantiser over those rows, byte
    for byte, and the planes split their block sums."""
    rng = np.random.default_rng(T + n)
    g = (rng.standard_normal((T, n)) * 1.5).astype(np.float32)
    u = (rng.standard_normal((T, n)) * rng.uniform(0.1, 4.0, (T, 1))).astype(np.float32)
    blk, bh, bl, ph, pl, _ = be.act_q8k_planes(2, g, u)
    y = be.swiglu(g.reshape(-1), u.reshape(-1)).reshape(T, n)
    ref = (oq.silu(g) * u).astype(np.float32)
    assert np.abs(y - ref).max() <= 2e-5 * np.abs(ref).max()
    print(f"swiglu rows T {T} n {n}: {int((y != ref).sum())} of {y.size} values differ from the oracle's in the last place")
    check_planes(blk, bh, bl, n, (T, n))
    assert np.array_equal(bh, ph) and np.array_equal(bl, pl)
    for t in range(T):
        assert np.array_equal(blk[t], oq.quantize(Q8_K, y[t])), (T, n, t)


def planes_step_cases():
    """Two shapes of tests/attn_seq_cases.py's batched-step table whose rows are whole Q8_K blocks: the smallest and the largest batch."""
    ok = [c for c in ac.step_cases() if (c.H * c.D) % 256 == 0]
    ok.sort(key=lambda c: c.T)
    return [ok[0], ok[-1]]


@pytest.mark.parametrize("c", planes_step_cases(), ids=lambda c: c.id)
def test_attention_merge_planes(be, c):
    """The merge behind the decode attention (attn.hip) writes attn_output's Q8_K rows and their bh / bl planes; mode 3 takes the quantiser's launch.  The
    planes against the block sums of the rows returned beside them, and rows and attention the bits of the entry without the planes."""
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, kc0, vc0, _ = ac.step_inputs(c)
    n = c.H * c.D
    for mode in c.modes:
        args = (mode, q, k_new, v_new, c.H, c.G, c.D, c.tk, kc0, c.tv, vc0, c.n_kv, cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, BASE, c.n_rot, c.neox, c.scale)
        att, _, _, blk, bh, bl = be.attn_batch_step(*args, want_planes=True)
        att0, _, _, blk0 = be.attn_batch_step(*args, want_q8k=True)
        assert np.array_equal(att.view(np.uint32), att0.view(np.uint32)) and np.array_equal(blk, blk0), (c.id, mode)
        check_planes(blk, bh, bl, n, (c.id, mode))
        for t in range(att.shape[0]):
            assert np.array_equal(blk[t], oq.quantize(Q8_K, att[t])), (c.id, mode, t)
