"""The grouped-expert prompt launches op by op (mi355_op_moe_mul_mat_grouped): launch_mmq_planes_moe, launch_mmq_planes_swiglu_moe and launch_mmq_q80_moe on the
cases of tests/moe_grouped_cases.py - second and third tiles of one expert, batches of 255 / 256 / 257 rows, idle token halves, one-row batches, slot counts at
their bound, more than eight row tiles, up to 256 experts.  Per case: every expert's batch against the CPU reference at that batch's own scale, the same bits
as the dense launch of the same kernel body, and nothing written outside [R][N] (tests/test_moe_grouped_cpu.py shows the table reaches those edges and that
the reference tells neighbouring experts apart)."""
import numpy as np
import pytest

import moe_grouped_cases as mc
from moe_grouped_cases import CASES, GUARD_ROWS

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(be, c, inp, tiles=0):
    be.set_option("mmq_q80_tiles", tiles)
    try:
        return be.moe_mul_mat_grouped(c["type"], c["form"], inp["W"], c["n_expert"], c["N"], c["K"], inp["x"], inp["counts"], ld_out=c["ld_out"], guard_rows=GUARD_ROWS)
    finally:
        be.set_option("mmq_q80_tiles", 0)


def check_values(c, inp, ref, ys, what=""):
    """Expert by expert, each batch against its own scale; the MXFP4 forms bit for bit."""
    N, worst = c["N"], 0.0
    for y, r in zip(ys, ref):
        for e in np.flatnonzero(inp["counts"]):
            o, n = int(inp["offs"][e]), int(inp["counts"][e])
            ye, re_ = y[o:o + n, :N], r[o:o + n]
            assert np.isfinite(ye).all(), (c["name"], what, int(e))
            if c["form"] >= 2:
                assert np.array_equal(bits(ye), bits(re_)), (c["name"], what, int(e), n, float(np.abs(ye - re_).max()))
            else:
                err, scale = float(np.abs(ye - re_).max()), float(np.abs(re_).max())
                worst = max(worst, (err - 1e-6) / scale)
                assert err <= mc.bound(c, re_), (c["name"], what, int(e), n, err, scale)
    return worst


def check_nothing_else_written(c, inp, ys, what=""):
    """Pad columns N .. ld_out of every row and all guard rows still hold the 0xFF bytes they were given; no element inside [R][N] does."""
    R, N = inp["R"], c["N"]
    for y in ys:
        u = bits(y)
        assert u.shape == (R + GUARD_ROWS, c["ld_out"])
        assert (u[:R, N:] == SENTINEL).all(), (c["name"], what, "pad columns")
        assert (u[R:] == SENTINEL).all(), (c["name"], what, "guard rows")
        assert not (u[:R, :N] == SENTINEL).any(), (c["name"], what, "unwritten results")


@pytest.mark.parametrize("c", [c for c in CASES if c["form"] < 2], ids=lambda c: c["name"])
def test_plane_forms(be, c):
    inp, ref = mc.prepared(c["name"])
    ys = launch(be, c, inp)
    check_nothing_else_written(c, inp, ys)
    worst = check_values(c, inp, ref, ys)
    print(f"{c['name']}: worst (|y - ref| - 1e-6) / max|ref_e| = {worst:.3g} (bound {mc.tol_rel(c):.0e})")
    # the same bits as the dense launch of the same body over that expert's tensor and rows ("planes2_body unchanged")
    N, K, t = c["N"], c["K"], c["type"]
    for name, v in (("mmq_planes", 1), ("mmq_tiles", 4), ("mmq_split", 1), ("mmq_ksplit", 0)):
        be.set_option(name, v)
    try:
        for e in np.flatnonzero(inp["counts"]):
            o, n = int(inp["offs"][e]), int(inp["counts"][e])
            xe = inp["x"][o:o + n]
            if c["form"] == 0:
                if n < 32:                                       # (the dense entry hands a shorter batch to the mat-vec)
                    continue
                dense = be.mul_mat(t, mc.expert_weights(c, inp["W"][0], e), N, K, xe)
            else:
                dense = be.ffn_gate_up(t, mc.expert_weights(c, inp["W"][0], e), mc.expert_weights(c, inp["W"][1], e), N, K, xe)
            assert np.array_equal(bits(ys[0][o:o + n, :N]), bits(dense)), (c["name"], int(e), n, float(np.abs(ys[0][o:o + n, :N] - dense).max()))
    finally:
        for name, v in (("mmq_planes", 1), ("mmq_tiles", 0), ("mmq_split", 0), ("mmq_ksplit", 1)):
            be.set_option(name, v)


@pytest.mark.parametrize("c", [c for c in CASES if c["form"] >= 2], ids=lambda c: c["name"])
def test_copy_forms(be, c):
    """Every token tile (32, 64, 128 rows and the launcher's choice): the restatement's bits for every batch length from 1, in both segments."""
    inp, ref = mc.prepared(c["name"])
    for tiles in mc.TILES_Q80:
        ys = launch(be, c, inp, tiles)
        assert len(ys) == (2 if c["form"] == 3 else 1)
        check_nothing_else_written(c, inp, ys, tiles)
        check_values(c, inp, ref, ys, tiles)


def test_refusals(be, pkg):
    """Shapes the launches' own predicates refuse, and counts that do not describe R rows: MI355_ERR_ARG, nothing launched."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((8, 512)).astype(np.float32)
    W = np.zeros(2 * 256 * 512, np.uint8)                        # (room for any of the shapes below)
    ok = [3, 5]

    def call(t, form, N, K, counts, R=None):
        return be.moe_mul_mat_grouped(t, form, [W, W], 2, N, K, x[:, :K], counts, R=R)

    for form in (0, 1):
        with pytest.raises(pkg.MI355Error):
            call(mc.Q4_K, form, 192, 256, ok)                    # N no multiple of 128
        with pytest.raises(pkg.MI355Error):
            call(mc.Q4_K, form, 64, 256, ok)
        with pytest.raises(pkg.MI355Error):
            call(mc.Q6_K, form, 128, 384, ok)                    # a plane type, K no multiple of 256
    for form in (2, 3):
        with pytest.raises(pkg.MI355Error):
            call(mc.Q4_K, form, 128, 256, ok)                    # the copy form takes MXFP4 only
        with pytest.raises(pkg.MI355Error):
            call(mc.MXFP4, form, 192, 256, ok)
    for form, t in ((0, mc.Q4_K), (1, mc.Q5_K), (2, mc.MXFP4), (3, mc.MXFP4)):
        for counts in ([3, 4], [3, 6], [9, -1], [0, 0]):         # one short, one over, a negative count, none at all
            with pytest.raises(pkg.MI355Error):
                call(t, form, 128, 256, counts)
        with pytest.raises(pkg.MI355Error):
            call(t, form, 128, 256, ok, R=7)
        ys = call(t, form, 128, 256, ok)                         # (and the same call with counts that do add up goes through)
        assert np.isfinite(ys[0][:8]).all()
