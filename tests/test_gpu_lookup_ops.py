"""The prompt-lookup draft kernel (csrc/lookup.hip) through mi355_op_ngram_draft against the rule in Python: the number of drafted tokens, the tokens and
(m, e) are compared for equality, on hand-built histories, the smallest at which the kernel can go wrong.  The kernel's constants, restated on purpose (NG_TILE,
NG_PART_MIN_TILES): a tile is 1024 token indices i = e - 1; a launch is one part up to len = 2049 and two parts of two tiles from len = 2050 on, so the first
tile boundary lies between i = 1023 and 1024, the first part boundary between i = 2047 and 2048."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TILE, PART, GRAM = 1024, 2048, [4, 5, 4, 4]              # GRAM: planted once among random symbols 0 .. 3 and again as the tail


def ngram_rule(h, ngram_min, ngram_max, k):
    """(draft, m, e): m(e) = tokens that agree walking back from h[e - 1] against h[-1], at most ngram_max, stopping at index 0; the largest m wins, the
    largest e among equals (no agreement anywhere: m = 0 at e = len - 1; no e at all: (0, 0)); the draft is h[e : e + k] if m >= ngram_min."""
    n, best_m, best_e = len(h), 0, 0
    for e in range(1, n):
        m = 0
        while m < ngram_max and e - 1 - m >= 0 and h[e - 1 - m] == h[n - 1 - m]:
            m += 1
        if m >= best_m:
            best_m, best_e = m, e
    return ([int(t) for t in h[best_e:best_e + k]] if best_m >= ngram_min else []), best_m, best_e


def rnd(n, seed, a=4):
    return np.random.default_rng(seed).integers(0, a, n).astype(np.int32)


# (name, history, ngram_min, ngram_max, k)
CASES = [(f"short-{n}", [1] * n, 2, 4, 8) for n in (0, 1, 2, 3)] + [
    ("periodic-abab", [0, 1] * 10, 2, 4, 8),                  # the best repeat overlaps the tail; two tokens follow it
    ("periodic-aaaa", [2] * 9, 2, 4, 8),
    ("periodic-16", [0, 1, 2] * 20, 16, 16, 16),
    ("straddles-tile", np.r_[rnd(TILE - 2, 1), GRAM, rnd(470, 2), GRAM], 2, 4, 8),
    ("straddles-part", np.r_[rnd(PART - 2, 3), GRAM, rnd(950, 4), GRAM], 2, 4, 8),
    ("only-at-e1", [4, 0, 1, 2, 3, 4], 1, 4, 16),
    ("cut-at-index-0", [0, 1, 2, 3, 0, 1], 2, 4, 16),
    ("late-fewer-than-k", [3, 0, 1, 2, 0, 1], 2, 4, 16),
    ("longer-beats-recent", [0, 1, 2, 3, 4, 5, 2, 3, 0, 1, 2, 3], 2, 4, 4),
    ("recent-beats-old", [1, 2, 3, 4, 1, 2, 3, 5, 1, 2, 3], 2, 4, 4),
    ("no-match", [0, 1, 2, 3, 4, 5], 1, 4, 4),
    ("below-ngram-min", [0, 1, 2, 3, 1, 5, 0, 4, 1], 2, 4, 4),       # the last token repeats, nothing longer: (m, e) = (1, 5) is reported, nothing drafted
    ("ngram-max-1-k-1", rnd(300, 3), 1, 1, 1),
] + [(f"len-{n}", rnd(n, n, 2), 1, 16, 16) for n in (TILE - 1, TILE, TILE + 1, TILE + 2, PART, PART + 1, PART + 2)] + [
    ("largest-grid", np.arange(131072, dtype=np.int32) % 5, 2, 16, 16),
]


def expect(h, ngram_min, ngram_max, k):
    draft, m, e = ngram_rule(h, ngram_min, ngram_max, k)
    return draft + [-1] * (16 - len(draft)), len(draft), [m, e]


def got(pkg, rows, lens, ngram_min, ngram_max, k):
    draft, nd, match = pkg.Backend().ngram_draft(rows, lens, ngram_min, ngram_max, k)
    return [(draft[s].tolist(), int(nd[s]), match[s].tolist()) for s in range(len(lens))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_draft_equals_the_rule(pkg, case):
    _, h, ngram_min, ngram_max, k = case
    h = np.asarray(h, np.int32)
    row = np.concatenate([h, np.full(3, 4, np.int32)])[None, :]            # cap > len: what lies behind a history is not part of it
    assert got(pkg, row, [h.size], ngram_min, ngram_max, k)[0] == expect(h, ngram_min, ngram_max, k)


def test_64_sequences_in_one_launch_do_not_see_each_other(pkg):
    lens = [0, 1, 2, 3, 5, 17, 64, 255] + [257 + 41 * s for s in range(52)] + [TILE + 1, PART + 2, 2500, 2499]
    rows = np.full((64, 2501), 1, np.int32)                                # a cap that is no multiple of 4: the rows start unaligned on the host
    for s, n in enumerate(lens):
        rows[s, :n] = rnd(n, 100 + s, 3)
    batch = got(pkg, rows, lens, 2, 5, 7)
    for s, n in enumerate(lens):
        assert batch[s] == expect(rows[s, :n], 2, 5, 7), s
        assert batch[s] == got(pkg, rows[s:s + 1, :max(n, 1)], [n], 2, 5, 7)[0], s


@pytest.mark.parametrize("kw,word", [
    (dict(n_seq=65), "n_seq"), (dict(cap=0), "cap"), (dict(lens=[9]), "length"), (dict(lens=[-1]), "length"), (dict(ngram_min=0), "ngram_min"),
    (dict(ngram_min=5), "ngram_min"), (dict(ngram_max=17), "ngram_max"), (dict(k=0), "k 0"), (dict(k=17), "k 17"), (dict(null=True), "null"),
])
def test_argument_errors_are_refused_by_word(pkg, kw, word):
    be = pkg.Backend()
    n_seq, cap = kw.get("n_seq", 1), kw.get("cap", 8)
    rows, lens = np.zeros((n_seq, cap), np.int32), np.asarray(kw.get("lens", [cap] * n_seq), np.int32)
    with pytest.raises(pkg.MI355Error, match=word):
        if kw.get("null"):
            out = np.zeros(16, np.int32)
            be._chk(be.lib.mi355_op_ngram_draft(rows.ctypes.data, 1, cap, None, 2, 4, 8, out.ctypes.data, out.ctypes.data, out.ctypes.data), "op_ngram_draft")
        be.ngram_draft(rows, lens, kw.get("ngram_min", 2), kw.get("ngram_max", 4), kw.get("k", 8))
