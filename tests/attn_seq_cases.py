"""Cases and oracle references of the multi-sequence attention tests (tests/test_gpu_attn_seq.py), shared with the CPU check of the cases themselves
(tests/test_attn_seq_cpu.py).  A cache holds cells of several sequences; a query of sequence s at position p sees cell c iff

    cell_pos[c] >= 0  and  cell_pos[c] <= p  and  (cell_seq[c] >> s) & 1  and  c < n_kv

and the reference is the oracle chained in the op's order: oq.rope, oq.quantize of the new rows (steps only), oq.flash_attn over that cell list.  The same
function restates the rule three ways wrong (MUTANTS); a case is only kept if each wrong rule moves a row the GPU test checks by 100 x its tolerance."""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

import np_twin as tw
import oracle_py as oq
from oracle_py import F16, Q4_0, Q8_0

TNAME = {F16: "f16", Q8_0: "q8_0", Q4_0: "q4_0"}
TOL = 2e-5                                  # x max(1, |ref|.max()): test_flash_attn_prefill_matrix_cores / test_attn_step_decode_block
BASE = 500000.0
LAYOUTS = ("regions", "ragged", "interleaved", "shared", "shuffled")
MUTANTS = ("noseq", "subtile_seq", "subtile_pos")   # sequence ignored; any sequence of the 32-query sub-tile; causal bound = the sub-tile's largest position
CK, SUB = 32, 32                            # attn_prefill.hip: keys per chunk, queries per sub-tile


def crc(*a) -> int:
    return zlib.crc32("/".join(str(x) for x in a).encode())


def n_kv_of(n_cells: int) -> int:
    """Cells the kernels scan: three less than the cache holds (67, 597, 30, 297, 2097, 381, 4477: none a multiple of 32)."""
    return n_cells - 3


# ---------------------------------------------------------------- cell tables
def region_sizes(name: str, n_kv: int, n_seq: int, rng) -> list:
    if name == "regions":                                   # whole 64-cell chunks per sequence, the first ones take what is left over; the last one ends at n_kv
        nch = (n_kv + 63) // 64
        assert nch >= n_seq, "fewer 64-cell chunks than sequences"
        per = [nch // n_seq + (1 if r < nch % n_seq else 0) for r in range(n_seq)]
        sizes = [64 * p for p in per]
        sizes[-1] -= 64 * nch - n_kv
        return sizes
    base = n_kv // n_seq                                    # ragged: no boundary on a multiple of 32
    sizes, at = [], 0
    for r in range(n_seq - 1):
        b = at + base + (int(rng.integers(-5, 6)) if base > 70 else 0)
        while b % 32 == 0 or b % 32 == 31:
            b += 1
        sizes.append(b - at)
        at = b
    sizes.append(n_kv - at)
    return sizes


def make_layout(name: str, n_cells: int, n_kv: int, ids, rng, step: bool = False):
    """(cell_pos int32 [n_cells], cell_seq uint64 [n_cells], region start per sequence or None).  step: a batched step follows - sequence 0 holds 64 cells and
    sequence 1 63 where their regions are large enough, every region keeps a free cell behind its sequence."""
    n_seq = len(ids)
    pos = np.full(n_cells, -1, np.int32)
    seq = np.zeros(n_cells, np.uint64)
    bit = [np.uint64(1) << np.uint64(s) for s in ids]
    starts = None
    if name in ("regions", "ragged", "shuffled"):
        sizes = region_sizes("regions" if name == "regions" else "ragged", n_kv, n_seq, rng)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
        for r in range(n_seq):
            free = (1 + (r % 3 if r > 1 else 0)) if (step or name == "regions") else 0
            ln = sizes[r] - free if name != "regions" or step else int(sizes[r] * rng.uniform(0.6, 0.95))
            if step:
                first = 130 if (n_seq == 2 and name == "ragged") else 64      # (two ragged regions: a third chunk for the first list, so that the lists differ)
                ln = min(ln, first if r == 0 else 63 if r == 1 else int(rng.integers(1, max(2, min(sizes[r] - 1, 61)))))
            ln = max(ln, 0)
            c = np.arange(starts[r], starts[r] + ln)
            p = np.arange(ln)
            if name == "shuffled":                          # positions permuted inside windows of 48 cells; three cells carry positions nobody reaches
                for w in range(0, ln, 48):
                    p[w:w + 48] = rng.permutation(p[w:w + 48])
                p[rng.choice(ln, min(3, ln), replace=False)] += 100000
            pos[c] = p
            seq[c] = bit[r]
    elif name == "interleaved":
        used = n_kv - (n_seq if step else 0)
        i = np.arange(used)
        pos[:used] = i // n_seq
        seq[:used] = np.array(bit, np.uint64)[i % n_seq]
        pos[:used][rng.random(used) < 0.1] = -1             # holes keep their stale mask
        if step:                                            # sequences of different lengths: every third one ends one 64-cell chunk early, every third one two
            fc = used // 64
            for j in range(n_seq):
                if j % 3:
                    pos[:used][(i % n_seq == j) & (i >= 64 * (fc - j % 3))] = -1
    elif name == "shared":
        assert n_seq == 3
        P = 100 if n_kv >= 100 else 40 if n_kv > 60 else 2 * n_kv // 3   # the first P cells belong to ids[0] and ids[2], not ids[1] (a seq_cp of a common prefix)
        pos[:P] = np.arange(P)
        seq[:P] = bit[0] | bit[2]
        nxt = [P, 0, P]
        for blk, c0 in enumerate(range(P, n_kv, 8)):
            r = blk % 3
            c = np.arange(c0, min(c0 + 8, n_kv))
            pos[c] = nxt[r] + np.arange(c.size)
            seq[c] = bit[r]
            nxt[r] += c.size
    else:
        raise ValueError(name)
    assert (pos[n_kv:] == -1).all()
    return pos, seq, starts


@functools.lru_cache(maxsize=64)
def cache_rows(t: int, n: int, n_cells: int, n_kv: int, tag: str, vscale: bool):
    """Quantised rows [n_cells][row bytes] of seeded unit-normal values (V: each cell scaled by 0.2 .. 3); the cells from n_kv on hold rows of another seed at
    thirty times the scale, so a kernel that read one would be off by far."""
    rng = np.random.default_rng(crc("rows", t, n, n_cells, tag, vscale))
    x = rng.standard_normal((n_cells, n)).astype(np.float32)
    if vscale:
        x *= rng.uniform(0.2, 3.0, (n_cells, 1)).astype(np.float32)
    x[n_kv:] *= 30.0
    rows = np.stack([oq.quantize(t, r) for r in x])
    rows.setflags(write=False)
    return rows


# ---------------------------------------------------------------- visibility, right and wrong
def visible(cell_pos, cell_seq, n_kv: int, q_pos, q_seq, t: int, rule: str = "right") -> np.ndarray:
    """Cells query t sees.  rule: "right", or one of MUTANTS."""
    idx = np.arange(cell_pos.size)
    sub = range(SUB * (t // SUB), min(len(q_pos), SUB * (t // SUB) + SUB))
    bound = max(int(q_pos[i]) for i in sub) if rule == "subtile_pos" else int(q_pos[t])
    if rule == "noseq":
        in_seq = np.ones(cell_pos.size, bool)
    elif rule == "subtile_seq":
        m = np.uint64(0)
        for i in sub:
            m |= np.uint64(1) << np.uint64(int(q_seq[i]))
        in_seq = (cell_seq & m) != 0
    else:
        in_seq = ((cell_seq >> np.uint64(int(q_seq[t]))) & np.uint64(1)) == 1
    return np.nonzero((cell_pos >= 0) & (cell_pos <= bound) & in_seq & (idx < n_kv))[0].astype(np.int32)


def checked_rows(T: int, q_seq) -> list:
    """Every third row, the first, the last and every row next to a change of sequence."""
    rows = set(range(0, T, 3)) | {0, T - 1}
    for t in range(1, T):
        if q_seq[t] != q_seq[t - 1]:
            rows |= {t - 1, t}
    return sorted(rows)


def with_v_acc(tv: int):
    """The oracle accumulates an f16 V in f32 for these comparisons (test_attn_step_decode_block): context manager."""
    class _Ctx:
        def __enter__(self):
            oq.set_fa_v_acc_f32(1 if tv == F16 else 0)

        def __exit__(self, *a):
            oq.set_fa_v_acc_f32(0)
    return _Ctx()


# ---------------------------------------------------------------- launch_flash_attn cases (prompt kernel, split kernel, parity kernel)
@dataclasses.dataclass(frozen=True)
class FaCase:
    kind: str                      # "prefill" (T >= 32, matrix cores), "split" (T < 32), "parity" (fa_v_acc_f16)
    D: int
    R: int
    tk: int
    tv: int
    n_cells: int
    layout: str
    T: int
    G: int = 2
    bump: int = 0

    @property
    def H(self) -> int:
        return self.G * self.R

    @property
    def id(self) -> str:
        return f"{self.kind}-D{self.D}R{self.R}-{TNAME[self.tk]}-{TNAME[self.tv]}-c{self.n_cells}-{self.layout}-T{self.T}"

    @property
    def ids(self):
        return (0, 1, 63) if self.layout == "shared" else (0, 1, 2)

    @property
    def n_kv(self) -> int:
        return n_kv_of(self.n_cells)

    @property
    def scale(self) -> float:
        return float(1 / np.sqrt(self.D))


def sub_tiles(R: int) -> int:
    return 4 if R == 1 else 2 if R == 2 else 1             # attn_prefill.hip fa_sub_tiles


def prefill_T(R: int) -> int:
    """One full workgroup tile, one full sub-tile and 5 queries: a ragged sub-tile and (R <= 2) sub-tiles without queries."""
    return 32 * sub_tiles(R) + 32 + 5


def prefill_cases() -> list:
    forms = [(64, R, t) for R in (1, 2, 4, 8) for t in (Q8_0, F16)] + [(128, R, t) for R in (3, 5, 6, 7) for t in (Q8_0, F16)]
    forms += [(128, R, Q4_0) for R in (1, 2, 8)] + [(128, R, Q8_0) for R in (1, 2, 4, 8)]
    out = []
    for (D, R, t) in forms:
        for n_cells in (70, 600):
            # 70 cells are two 64-cell chunks: no room for three aligned regions; every layout at 600 on R = 1 and R = 4
            lays = ("interleaved", "shared") if (n_cells == 70 or R not in (1, 4)) else LAYOUTS
            out += [FaCase("prefill", D, R, t, t, n_cells, lay, prefill_T(R)) for lay in lays]
    return out


def split_cases() -> list:
    """The split kernel at T = 1, 5, 31: every (R, D, type pair), the other dimensions cycled over them so that each value meets each of the others' often."""
    pairs = ((F16, F16), (Q8_0, Q8_0), (Q4_0, Q4_0), (Q8_0, F16), (F16, Q8_0))
    out, i = [], 0
    for R in (2, 3, 5, 6, 7):
        for D in (64, 128):
            for (tk, tv) in pairs:
                out.append(FaCase("split", D, R, tk, tv, (33, 300)[(i // 3) % 2], ("interleaved", "shared", "shuffled")[(i + i // 6) % 3], (1, 5, 31)[i % 3]))
                i += 1
    out.append(FaCase("split", 128, 3, Q8_0, Q8_0, 2100, "shuffled", 5))        # more than one 1024-cell split
    out.append(FaCase("split", 128, 5, Q8_0, Q8_0, 300, "regions", 1))          # whole splits hold only other sequences' cells
    out.append(FaCase("parity", 128, 3, F16, F16, 300, "shared", 5))
    return out


def fa_inputs(c: FaCase):
    """cell_pos, cell_seq, q_pos, q_seq, q [T][H][D], K rows, V rows."""
    rng = np.random.default_rng(crc(c.id, "in" + "+" * c.bump))
    cell_pos, cell_seq, _ = make_layout(c.layout, c.n_cells, c.n_kv, c.ids, rng)
    P = []                                                       # sorted visible-capable positions per sequence
    for s in c.ids:
        m = (cell_pos >= 0) & (((cell_seq >> np.uint64(s)) & np.uint64(1)) == 1) & (cell_pos < 50000)
        P.append(np.sort(cell_pos[m]))
    T = c.T
    q_pos = np.zeros(T, np.int32)
    q_seq = np.zeros(T, np.int32)

    def draw(j, lo_q, hi_q, n):
        p = P[j]
        lo, hi = int(p[int(lo_q * (p.size - 1))]), int(p[int(hi_q * (p.size - 1))])
        return rng.integers(lo, hi + 1, n)
    if c.kind == "prefill":
        t0 = T - 37                                              # the full tile: one sequence, positions high enough to leave whole chunks below all of them
        q_seq[:t0], q_pos[:t0] = c.ids[0], draw(0, 0.7, 1.0, t0)
        q_pos[0] = draw(0, 0.7, 0.7, 1)[0]
        q_seq[t0:t0 + 16], q_pos[t0:t0 + 16] = c.ids[1], draw(1, 0.0, 0.5, 16)     # the full sub-tile: two sequences
        q_seq[t0 + 16:t0 + 32], q_pos[t0 + 16:t0 + 32] = c.ids[2], draw(2, 0.0, 0.5, 16)
        q_seq[t0 + 32:], q_pos[t0 + 32:] = c.ids[0], draw(0, 0.0, 0.25, 5)         # the ragged one
    else:
        for t in range(T):
            j = t % 3 if T > 1 else 0
            q_seq[t], q_pos[t] = c.ids[j], draw(j, 0.0, 1.0, 1)[0]
        q_pos[T - 1] = P[list(c.ids).index(int(q_seq[T - 1]))][-1]                # one query sees its whole sequence
    q = rng.standard_normal((T, c.H, c.D)).astype(np.float32)
    n = c.G * c.D
    return cell_pos, cell_seq, q_pos, q_seq, q, cache_rows(c.tk, n, c.n_cells, c.n_kv, "k", False), cache_rows(c.tv, n, c.n_cells, c.n_kv, "v", True)


def fa_reference(c: FaCase, inp, rows, rule: str = "right") -> dict:
    cell_pos, cell_seq, q_pos, q_seq, q, kc, vc = inp
    out = {}
    with with_v_acc(c.tv):
        for t in rows:
            cells = visible(cell_pos, cell_seq, c.n_kv, q_pos, q_seq, t, rule)
            out[t] = oq.flash_attn(q[t], c.H, c.G, c.D, c.tk, kc, c.tv, vc, cells, c.scale) if cells.size else None
    return out


def prefill_structure(c: FaCase, inp) -> dict:
    """Counts of what the prompt kernel's tile-wide shortcuts can get wrong, over the case's workgroup tiles (32 * sub_tiles(R) queries) and 32-cell chunks."""
    cell_pos, cell_seq, q_pos, q_seq, *_ = inp
    T, TQ = c.T, 32 * sub_tiles(c.R)
    mixed = sum(1 for s0 in range(0, T, SUB) if len(set(q_seq[s0:s0 + SUB].tolist())) > 1 and len(q_seq[s0:s0 + SUB]) == SUB)
    n_open = n_partial = n_none = n_mixed = 0
    for t0 in range(0, T, TQ):
        qs = range(t0, min(T, t0 + TQ))
        tile_seqs = np.uint64(0)
        for t in qs:
            tile_seqs |= np.uint64(1) << np.uint64(int(q_seq[t]))
        minpos = min(int(q_pos[t]) for t in qs)
        for ch in range((c.n_kv + CK - 1) // CK):
            cells = np.arange(ch * CK, min((ch + 1) * CK, c.n_kv))
            cp, cs = cell_pos[cells], cell_seq[cells]
            if not (cp >= 0).any():
                continue
            if cells.size == CK and (cp >= 0).all() and (cp <= minpos).all() and ((cs & tile_seqs) == tile_seqs).all():
                n_open += 1
            sees = [bool(((cp >= 0) & (cp <= q_pos[t]) & (((cs >> np.uint64(int(q_seq[t]))) & np.uint64(1)) == 1)).any()) for t in qs]
            # visible to some queries of the tile but not all, by sequence: a query that sees none of the chunk although one of its cells lies at or below
            # the query's position - the position alone would not hide it
            if any(sees) and any((not v) and bool(((cp >= 0) & (cp <= q_pos[t])).any()) for v, t in zip(sees, qs)):
                n_partial += 1
            if not any(sees):
                n_none += 1
            # ... and the same inside a chunk: a query sees one of its cells while another cell at or below its position belongs to another sequence
            for t in qs:
                mine = (cp >= 0) & (cp <= q_pos[t])
                own = ((cs >> np.uint64(int(q_seq[t]))) & np.uint64(1)) == 1
                if (mine & own).any() and (mine & ~own).any():
                    n_mixed += 1
                    break
    return {"mixed_sub_tiles": mixed, "open": n_open, "partial_by_seq": n_partial, "invisible": n_none, "mixed_chunks": n_mixed}


# ---------------------------------------------------------------- the batched single-token step
Q_TIE = 2e-5   # see tie_free_queries


def tie_free_queries(rng, T: int, H: int, D: int, pos, n_rot: int, neox: bool) -> np.ndarray:
    """Unit-normal un-rotated queries [T][H * D] none of whose ROTATED elements lies within Q_TIE of a q8_0 rounding tie.  The step kernels rotate q themselves
    and quantise it to q8_0 for the dot with a quantised K; a device cosf / sinf may move a rotated value by 4e-6 (tests/test_gpu_ops.py::test_rope) and the
    block maximum, hence the step d = amax / 127, by as much - up to 127 * 4e-6 / amax of a code, 8e-6 at the unit scale of these inputs.  An element that
    close to x / d = k + 0.5 takes the other code on the device: one step of amax / 127 = 0.02 in one factor of one score, which moves a row by ~1e-3 - the
    oracle's distance from the device's rope, not the attention kernel's error.  Heads that hold such an element are drawn again."""
    q = rng.standard_normal((T, H, D)).astype(np.float32)
    for t in range(T):
        for h in range(H):
            for _ in range(100):
                x = oq.rope(q[t, h], 1, D, int(pos[t]), BASE, neox=neox, n_rot=n_rot).reshape(D // 32, 32).astype(np.float64)
                d = np.abs(x).max(axis=1, keepdims=True) / 127
                f = x / d
                if (np.abs(np.abs(f - np.floor(f)) - 0.5) * d > Q_TIE).all():
                    break
                q[t, h] = rng.standard_normal(D).astype(np.float32)
            else:
                raise AssertionError("no tie-free head in 100 draws")
    return q.reshape(T, H * D)


@dataclasses.dataclass(frozen=True)
class StepCase:
    D: int
    R: int
    tk: int
    tv: int
    T: int
    n_cells: int
    layout: str
    rope: str = "norm"             # "norm", "neox" (the whole head), "rot64" (NORM, 64 of 128 rotated)
    bump: int = 0

    @property
    def G(self) -> int:
        return 1024 // self.D      # G * D = 1024: what the small-batch store takes

    @property
    def H(self) -> int:
        return self.G * self.R

    @property
    def n_rot(self) -> int:
        return 64 if self.rope == "rot64" else self.D

    @property
    def neox(self) -> bool:
        return self.rope == "neox"

    @property
    def n_kv(self) -> int:
        return n_kv_of(self.n_cells)

    @property
    def scale(self) -> float:
        return float(1 / np.sqrt(self.D))

    @property
    def id(self) -> str:
        return f"step-D{self.D}R{self.R}-{TNAME[self.tk]}-{TNAME[self.tv]}-T{self.T}-c{self.n_cells}-{self.layout}-{self.rope}"

    @property
    def ids(self):
        return tuple(range(64)) if self.T == 64 else (0, 63) if self.T == 2 else (0, 1, 2, 40, 63)

    @property
    def modes(self):
        """The launch forms that have a kernel for the case (mi355_op_attn_batch_step refuses the others)."""
        lists = not self.neox and Q4_0 not in (self.tk, self.tv)
        return (0, 1, 2, 3) if lists else (0, 3)


def step_cases() -> list:
    """Every (head form, cache pair); batch size, layout and rope cycle so that each batch size meets every rope and every layout."""
    forms = [(128, R) for R in (1, 2, 4, 8, 3, 7)] + [(64, 1), (64, 4)]
    out, i = [], 0
    for (D, R) in forms:
        pairs = [(F16, F16), (Q8_0, Q8_0)] + ([(Q8_0, F16), (F16, Q8_0)] if R in (1, 2, 4, 8) else []) + ([(Q4_0, Q4_0)] if D == 128 and R in (1, 2, 4, 8) else [])
        for (tk, tv) in pairs:
            T = (2, 5, 64)[i % 3]
            lay = "interleaved" if T == 64 else ("regions", "ragged", "interleaved")[(i // 3 + i) % 3]
            rope = ("norm", "neox", "rot64" if D == 128 else "norm")[(i // 3) % 3]
            out.append(StepCase(D, R, tk, tv, T, 384, lay, rope))
            i += 1
    out.append(StepCase(128, 4, Q8_0, Q8_0, 64, 4480, "regions"))              # 70 chunks: more than 64 splits for the merge in mode 0
    return out


def step_inputs(c: StepCase):
    """cell_pos / cell_seq with the new cells set, tok_pos, tok_seq, tok_cell, q, k_new, v_new, K rows, V rows (before the step), region starts or None."""
    rng = np.random.default_rng(crc(c.id, "in" + "+" * c.bump))
    ids = c.ids
    cell_pos, cell_seq, starts = make_layout(c.layout, c.n_cells, c.n_kv, ids, rng, step=True)
    T = c.T
    empty_seq = T - 1 if T > 2 else None                        # a sequence without an earlier cell (T = 2: both lists are needed for the other properties)
    bit = [np.uint64(1) << np.uint64(s) for s in ids]
    if empty_seq is not None:
        cell_pos[cell_seq == bit[empty_seq]] = -1
    tok_pos, tok_cell = np.zeros(T, np.int32), np.zeros(T, np.int32)
    for j in range(T):
        mine = np.nonzero((cell_pos >= 0) & (cell_seq == bit[j]))[0]
        tok_pos[j] = int(cell_pos[mine].max()) + 1 if mine.size else 0
        if starts is not None:
            tok_cell[j] = starts[j] + (int(mine.max()) + 1 - starts[j] if mine.size else 0)
        elif c.layout == "interleaved":
            tok_cell[j] = 63 if j == 63 % T else c.n_kv - T + j            # cell 63: the last of its chunk (a hole of the token's own residue class)
    for j in range(T):                                          # a stale cell of a later position in the token's own sequence, at or below the largest
        mine = np.nonzero((cell_pos >= 0) & (cell_seq == bit[j]))[0]   # position of the token's group of 32: never visible to it
        top = int(tok_pos[32 * (j // 32):32 * (j // 32) + 32].max())
        if mine.size >= 3 and tok_pos[j] < top:
            cell_pos[rng.choice(mine[:-1])] = int(rng.integers(tok_pos[j] + 1, top + 1))
    assert len(set(tok_cell.tolist())) == T and (tok_cell < c.n_kv).all()
    for j in range(T):
        assert cell_pos[tok_cell[j]] == -1 or (c.layout == "interleaved" and tok_cell[j] == 63), (c.id, j)
        cell_pos[tok_cell[j]] = tok_pos[j]
        cell_seq[tok_cell[j]] = bit[j]
    tok_seq = np.array(ids, np.int32)
    n = c.G * c.D
    q = tie_free_queries(rng, T, c.H, c.D, tok_pos, c.n_rot, c.neox)
    k_new = rng.standard_normal((T, n)).astype(np.float32)
    v_new = (rng.standard_normal((T, n)) * 1.7).astype(np.float32)
    return (cell_pos, cell_seq, tok_pos, tok_seq, tok_cell, q, k_new, v_new, cache_rows(c.tk, n, c.n_cells, c.n_kv, "k", False),
            cache_rows(c.tv, n, c.n_cells, c.n_kv, "v", True), starts)


def step_new_rows(c: StepCase, inp):
    """The oracle's rotated q [T][H * D], rotated K rows f32 [T][G * D] and the quantised K / V rows of the new cells."""
    _, _, tok_pos, _, _, q, k_new, v_new, *_ = inp
    qr = np.stack([oq.rope(q[t], c.H, c.D, int(tok_pos[t]), BASE, neox=c.neox, n_rot=c.n_rot).reshape(-1) for t in range(c.T)])
    kr = np.stack([oq.rope(k_new[t], c.G, c.D, int(tok_pos[t]), BASE, neox=c.neox, n_rot=c.n_rot).reshape(-1) for t in range(c.T)])
    return qr, kr, np.stack([oq.quantize(c.tk, r) for r in kr]), np.stack([oq.quantize(c.tv, r) for r in v_new])


def step_reference(c: StepCase, inp, qr, kc_after, vc_after, rows, rule: str = "right") -> dict:
    """Attention rows over the cache AFTER the store (the caller passes the oracle's rows, or the ones the device wrote: what its attention saw)."""
    cell_pos, cell_seq, tok_pos, tok_seq = inp[:4]
    out = {}
    with with_v_acc(c.tv):
        for t in rows:
            cells = visible(cell_pos, cell_seq, c.n_kv, tok_pos, tok_seq, t, rule)
            out[t] = oq.flash_attn(qr[t].reshape(c.H, c.D), c.H, c.G, c.D, c.tk, kc_after, c.tv, vc_after, cells, c.scale).reshape(-1)
    return out


def step_structure(c: StepCase, inp) -> dict:
    cell_pos, cell_seq, tok_pos, tok_seq, tok_cell = inp[:5]
    starts = inp[-1]
    nch = (c.n_kv + 63) // 64
    empty_pairs, lens = 0, []
    for t in range(c.T):
        vis = visible(cell_pos, cell_seq, c.n_kv, tok_pos, tok_seq, t)
        has = set((vis // 64).tolist())
        empty_pairs += nch - len(has)
        occ = (cell_pos >= 0) & (((cell_seq >> np.uint64(int(tok_seq[t]))) & np.uint64(1)) == 1) & (np.arange(cell_pos.size) < c.n_kv)
        lens.append(len(set((np.nonzero(occ)[0] // 64).tolist())))
    rel = [int(tok_cell[t] - (starts[t] if starts is not None else 0)) for t in range(c.T)]
    return {"empty_pairs": empty_pairs, "list_lengths": lens, "edge_cells": sum(1 for r in rel if r in (63, 64)),
            "lone_tokens": sum(1 for t in range(c.T) if visible(cell_pos, cell_seq, c.n_kv, tok_pos, tok_seq, t).size == 1)}


# ---------------------------------------------------------------- single-token forms over a cache with other sequences' cells
def single_inputs(H: int, G: int, n_cells: int, layout: str, tkv: int, D: int = 128):
    """A single-token step of sequence ids[2] into a cache of three sequences: cell_pos / cell_seq with the new cell set, tok_pos, tok_seq, tok_cell, q, k_new,
    v_new, K rows, V rows."""
    ids = (0, 1, 63) if layout == "shared" else (0, 1, 2)
    rng = np.random.default_rng(crc("single", H, G, n_cells, layout, tkv))
    n_kv = n_kv_of(n_cells)
    cell_pos, cell_seq, _ = make_layout(layout, n_cells, n_kv, ids, rng)
    s = ids[2]
    mine = np.nonzero((cell_pos >= 0) & (((cell_seq >> np.uint64(s)) & np.uint64(1)) == 1))[0]
    tok_pos = int(cell_pos[mine].max()) + 1
    tok_cell = n_kv                                              # the first cell behind the occupied ones
    cell_pos[tok_cell], cell_seq[tok_cell] = tok_pos, np.uint64(1) << np.uint64(s)
    n = G * D
    q = {neox: tie_free_queries(rng, 1, H, D, [tok_pos], D, neox).reshape(H, D) for neox in (False, True)}   # (per rotary pairing: the NORM and the NEOX entry)
    k_new = rng.standard_normal(n).astype(np.float32)
    v_new = (rng.standard_normal(n) * 1.7).astype(np.float32)
    return cell_pos, cell_seq, tok_pos, s, tok_cell, q, k_new, v_new, cache_rows(tkv, n, n_cells, n_kv, "k", False), cache_rows(tkv, n, n_cells, n_kv, "v", True)


def rand_kquant_weights(rng, t: int, n_elems: int, dscale: float = 1e-2) -> np.ndarray:
    """Random 256-element K-quant blocks with block scales around dscale (tests/test_gpu_ops.py rand_weights): the attn_output weight of the single-token forms."""
    raw = rng.integers(0, 256, n_elems // 256 * {12: 144, 13: 176, 14: 210}[t], dtype=np.uint8)
    blk = raw.view(tw.DT[t])
    blk["d"] = (rng.uniform(0.5, 1.5, blk.size) * dscale).astype("<f2")
    if t in (12, 13):
        blk["dmin"] = (rng.uniform(0.5, 1.5, blk.size) * dscale).astype("<f2")
    return raw


def float64_attention(q_row, H, G, D, tk, kc, tv, vc, cells, scale):
    """float64 attention over the stored (quantised) K / V and the q as the kernel's dot sees it (tests/test_oracle_kat.py::test_flash_attn_vs_float64)."""
    n_ctx = kc.shape[0]
    kd = np.stack([oq.dequantize(tk, r, G * D) for r in kc]).astype(np.float64).reshape(n_ctx, G, D)
    vd = np.stack([oq.dequantize(tv, r, G * D) for r in vc]).astype(np.float64).reshape(n_ctx, G, D)
    qt = oq.vec_dot_type(tk)
    qd = np.stack([oq.dequantize(qt, oq.quantize(qt, q_row[h]), D) for h in range(H)]).astype(np.float64)
    out = np.zeros((H, D))
    for h in range(H):
        g = h // (H // G)
        s = kd[cells, g] @ qd[h] * scale
        w = np.exp(s - s.max())
        out[h] = (w[:, None] * vd[cells, g]).sum(0) / w.sum()
    return out
