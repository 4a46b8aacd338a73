"""nbg_group_by over the value domain: the cells tests/test_gpu_groupby.py's RMAT rows never hold.

The input is rowtable.value_table on the device (see tests/test_gpu_values_orderby.py for what it
holds) and, for the accumulators' identities, a numeric table built here.  Expected groups come
from rowtable.group_ref (numpy, written from include/nbg.h; pinned on the CPU by
tests/test_rowtable_model.py), never from the device; results are compared by bits with
rowtable.check_groups.  What include/nbg.h promises and these tests hold the device to: zeros of
both signs are one group and each NaN bit pattern its own; int64 SUM wraps and keeps the column's
type; AVG is double(wrapped sum) / n; MAX / MIN follow the column's order — over doubles with NaNs
that is the IEEE total-order image, so the highest positive NaN is the MAX and the lowest negative
NaN the MIN (the reference's answer there depends on its row order), and of zeros of both signs
either sign may be reported.

Double sums.  A group whose every summation order gives the same class (a NaN among the terms,
infinities of one sign, infinities of both) is compared by class and sign.  A finite group is
compared with math.fsum, the exactly rounded sum, within gamma_{n-1} * sum|x_i|,
gamma_k = k * 2^-53 / (1 - k * 2^-53): the bound of recursive summation in any order.  STD keeps
the relative n * 2^-52 rule of tests/test_gpu_groupby.py where its premise holds: both sides add
the same non-negative terms (x - avg)^2, which needs the same avg on both sides — an INT column
(the int64 sum is exact) or doubles whose sums are exact (multiples of 1/8 far below 2^53).

Accumulator identities.  k_gb_accum leaves out the flush of a workgroup's LDS partial that
equals the accumulator's identity, and a row's value can equal it: INT64_MIN under MAX (image 0),
INT64_MAX under MIN, -1 under BIT_AND, 0 under BIT_OR / BIT_XOR / SUM, -0.0 under a double SUM,
the lowest image (the all-ones NaN) under a double MAX and the highest (0x7FFF...F) under MIN.
A workgroup walks whole segments, so each case is run on the GO's own result — where a segment
holding nothing but group B's identity cells is asserted from nbg_rows_segment — and on its
ORDER BY pos copy, one segment that one workgroup walks alone."""
import numpy as np
import pytest

from nebula_amd import NbgError, _lib as L, expr as E
from tests.support import rowtable as rt

pytestmark = pytest.mark.gpu

GB_LDS_BYTES = 16 * 1024       # csrc/nbg_internal.h
COLUMNS = ["pos", "i", "x", "d", "s", "t", "b", "z", "c", "g"]


class Fixture:
    pass


@pytest.fixture(scope="module")
def vg():
    f = Fixture()
    f.t = rt.value_table()
    f.ld = rt.load_value_table(f.t)
    f.rows, f.cols = rt.go_checked(f.ld)
    assert len(f.ld.segments(f.rows)) >= 2
    f.digest = f.rows.digest()
    yield f
    assert f.rows.digest() == f.digest
    f.rows.free()
    f.ld.close()


def _group(f, keys, aggs, rows=None, idx=None, what=""):
    ref = rt.group_ref(f.t, keys, aggs, idx)
    cols, kinds = f.ld.group(f.rows if rows is None else rows, keys, aggs)
    rt.check_groups(cols, kinds, f.t, keys, ref, what or str(keys))
    return cols, ref


# ------------------------------------------------------------------------------ 1. keys
EXACT_AGGS = [("COUNT", None), ("SUM", "i"), ("AVG", "i"), ("MAX", "i"), ("MIN", "i"), ("MAX", "x"), ("MIN", "x"),
              ("MAX", "s"), ("MIN", "s"), ("MAX", "d"), ("MIN", "t"), ("MAX", "b"), ("SUM", "d"), ("SUM", "t"),
              ("BIT_AND", "i"), ("BIT_OR", "i"), ("BIT_XOR", "i"), ("COUNT_DISTINCT", "x"), ("SUM", "s"), ("AVG", "b"),
              ("BIT_XOR", "t"), ("STD", "d")]
KEYS = [["i"], ["x"], ["d"], ["s"], ["t"], ["b"], ["z"], ["c"], ["g"], ["pos"], ["x", "i"], ["s", "d"], []]


@pytest.mark.parametrize("keys", KEYS, ids=lambda k: "_".join(k) or "const")
def test_keys(vg, keys):
    assert vg.t.names == COLUMNS
    cols, ref = _group(vg, keys, EXACT_AGGS)
    if keys == ["x"]:
        x = vg.t.bits["x"].view(np.uint64)
        key, n = cols[0].view(np.uint64), cols[1]
        zero = np.nonzero((key == 0) | (key == np.uint64(1 << 63)))[0]
        assert len(zero) == 1 and n[zero[0]] == ((x == 0) | (x == np.uint64(1 << 63))).sum() >= 6      # zeros: one group
        for nan in rt.NANS:                                     # each NaN bit pattern: its own group
            at = np.nonzero(key == np.uint64(nan))[0]
            assert len(at) == 1 and n[at[0]] == (x == np.uint64(nan)).sum() >= 3
    if keys == ["z"]:
        assert len(cols[0]) == 1 and cols[1][0] == vg.t.n       # nothing but zeros of both signs
    if keys == ["s"]:
        assert vg.t.strings[0] == b"" and (cols[0] == 0).sum() == 1          # "" is a group
        assert len(cols[0]) == len(rt.STRS)
    if keys == ["d"]:
        assert set(cols[0].tolist()) == set(rt.VIDS)
    if keys in (["i"], ["pos"], ["x", "i"]):
        assert ref.n * 2 * 8 > GB_LDS_BYTES                     # (nacc >= 2) the accumulators outgrow the LDS


# ------------------------------------------------------------------------------ 2. identities
ALL_ONES, HIGHEST_IMAGE = 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF
IDENT_CASES = {                     # aggregate -> (column, the cell that equals its identity)
    "max_int64_min": ("MAX", "v", rt.INT64_MIN),
    "min_int64_max": ("MIN", "v", rt.INT64_MAX),
    "and_minus_1": ("BIT_AND", "v", -1),
    "or_0": ("BIT_OR", "v", 0),
    "xor_0": ("BIT_XOR", "v", 0),
    "sum_0": ("SUM", "v", 0),
    "dsum_neg_zero": ("SUM", "y", 1 << 63),
    "dmax_lowest_image": ("MAX", "y", ALL_ONES),
    "dmin_highest_image": ("MIN", "y", HIGHEST_IMAGE),
}
IDENT_AGGS = [("COUNT", None), ("MAX", "v"), ("MIN", "v"), ("BIT_AND", "v"), ("BIT_OR", "v"), ("BIT_XOR", "v"),
              ("SUM", "v"), ("SUM", "y"), ("MAX", "y"), ("MIN", "y")]
SIDE, RUN, FILLER = 300, 6000, 3000
CASE_ROWS = 5 + SIDE + RUN + SIDE + FILLER
CASE_SRC = 16                       # source indices per case


@pytest.fixture(scope="module")
def idt():
    """One numeric table, one block of rows per case: group A (key 1: five rows, every cell the
    identity), group B (key 2: SIDE ordinary rows, a run of RUN identity cells under one source —
    longer than the rows of several workgroups — and SIDE ordinary rows) and FILLER one-row groups
    that push the accumulators out of the LDS when their sources are part of the GO."""
    rng = np.random.default_rng(23)
    g, v, y, src = [], [], [], []
    for k, (_, col, ident) in enumerate(IDENT_CASES.values()):
        n = CASE_ROWS
        gk = np.concatenate([np.full(5, 1), np.full(2 * SIDE + RUN, 2), 1000 + np.arange(FILLER)])
        vk = rng.integers(rt.INT64_MIN, rt.INT64_MAX, n, endpoint=True)
        yk = (rng.integers(-(1 << 30), 1 << 30, n) / 8.0).view(np.uint64)     # exact sums in any order
        tgt = vk if col == "v" else yk
        tgt[:5] = np.array([ident], np.uint64 if col == "y" else np.int64)[0]
        tgt[5 + SIDE:5 + SIDE + RUN] = tgt[0]
        sk = np.concatenate([np.full(5, 0), np.full(SIDE, 1), np.full(RUN, 2), np.full(SIDE, 3),
                             4 + np.arange(FILLER) % 8]) + k * CASE_SRC
        g.append(gk), v.append(vk), y.append(yk), src.append(sk)
    f = Fixture()
    f.t = rt.Table([("g", rt.INT, np.concatenate(g)), ("v", rt.INT, np.concatenate(v)),
                    ("y", rt.DOUBLE, np.concatenate(y))], src=np.concatenate(src))
    f.ld = rt.load_numeric_table(f.t)
    yield f
    f.ld.close()


@pytest.mark.parametrize("many", [False, True], ids=["lds", "global"])
@pytest.mark.parametrize("case", list(IDENT_CASES))
def test_identity_collisions(idt, case, many):
    k = list(IDENT_CASES).index(case)
    fun, col, ident = IDENT_CASES[case]
    ident_bits = np.array([ident & ((1 << 64) - 1)], np.uint64).view(np.int64)[0]
    idx = idt.t.rows_of_sources(k * CASE_SRC, k * CASE_SRC + (CASE_SRC if many else 4))
    rows, cols = rt.go_checked(idt.ld, idx)
    try:
        ngroups = 2 + (FILLER if many else 0)
        assert (len(IDENT_AGGS) * ngroups * 8 <= GB_LDS_BYTES) == (not many)       # nacc = 10: COUNT + one each
        # the GO's segments: one holds nothing but group B's identity cells, and B lies in several
        b_segs, pure = 0, 0
        for at, n in idt.ld.segments(rows):
            in_b = cols["g"][at:at + n] == 2
            b_segs += bool(in_b.any())
            pure += bool(in_b.all() and (cols[col][at:at + n] == ident_bits).all())
        assert pure >= 1 and b_segs >= pure + 1, (pure, b_segs)
        ref = rt.group_ref(idt.t, ["g"], IDENT_AGGS, idx)
        for inp in (rows, idt.ld.by_pos(rows)):
            dev, kinds = idt.ld.group(inp, ["g"], IDENT_AGGS)
            rt.check_groups(dev, kinds, idt.t, ["g"], ref, case)
            # group A: the aggregate of nothing but identity cells is that cell
            a = int(np.nonzero(dev[0] == 1)[0][0])
            got = dev[1 + IDENT_AGGS.index((fun, col))][a]
            assert got == ident_bits, (case, hex(int(got) & ((1 << 64) - 1)))
            if inp is not rows:
                inp.free()
    finally:
        rows.free()


# ------------------------------------------------------------------------------ 3. wrapping
def _by_key(cols, key):
    return int(np.nonzero(cols[0] == key)[0][0])


def test_int_sums_wrap(vg):
    aggs = [("COUNT", None), ("SUM", "i"), ("AVG", "i"), ("STD", "i"), ("MAX", "i"), ("MIN", "i")]
    cols, ref = _group(vg, ["g"], aggs)       # STD: an INT column, so one avg on both sides (see the docstring)
    a, b = _by_key(cols, rt.G_WRAP_MAX), _by_key(cols, rt.G_WRAP_MIN)
    assert cols[1][a] == 3 and cols[2][a] == 0                               # INT64_MAX + INT64_MAX + 2 wraps to 0
    assert cols[3][a] == rt.dbits(0.0)
    assert cols[1][b] == 2 and cols[2][b] == rt.INT64_MAX                    # INT64_MIN + -1 wraps to INT64_MAX
    assert cols[3][b] == rt.dbits(float(rt.INT64_MAX) / 2)
    std = cols[4].view(np.float64)
    assert std[a] > 4e18 and std[b] > 6e18                                   # around the wrapped avg, as the reference


def test_sum_keeps_vid_and_timestamp(vg):
    """SUM over negative VIDs and over TIMESTAMPs wraps like any int64 and keeps the column's type:
    the result is an INT-kind column that AVG still refuses."""
    aggs = [("COUNT", None), ("SUM", "d"), ("SUM", "t"), ("SUM", "i")]
    ref = rt.group_ref(vg.t, ["b"], aggs)
    d, t = vg.t.bits["d"], vg.t.bits["t"]
    assert (d < 0).any() and abs(sum(t.tolist())) >= 1 << 63                 # negative vids; a sum that wraps
    out = vg.ld.group_rows(vg.rows, ["b"], aggs)
    try:
        names = ["b", "n", "sd", "st", "si"]
        cols = vg.ld.bits_of(out, names, [])
        kinds = vg.ld.kinds_of(out)
        rt.check_groups([cols[n] for n in names], kinds, vg.t, ["b"], ref)
        assert kinds == [L.V_BOOL, L.V_INT, L.V_INT, L.V_INT, L.V_INT]
        key = [E.input_prop("b").encode()]
        for col, ok in (("sd", False), ("st", False), ("si", True)):
            ys = [("AVG", E.input_prop(col).encode(), None)]
            if ok:
                again = vg.ld.eng.group_by(out, names, key, ys)
                assert again.count == 2
                again.free()
            else:
                with pytest.raises(NbgError) as ex:
                    vg.ld.eng.group_by(out, names, key, ys)
                assert ex.value.code == L.E_UNSUPPORTED
    finally:
        out.free()


# ------------------------------------------------------------------------------ 4. doubles
def test_double_aggregates(vg):
    aggs = [("COUNT", None), ("SUM", "x"), ("AVG", "x"), ("MAX", "x"), ("MIN", "x")]
    cols, ref = _group(vg, ["g"], aggs)
    s, avg, mx, mn = (cols[k].view(np.float64) for k in (2, 3, 4, 5))
    at = {g: _by_key(cols, g) for g in (201, 202, 203, 204, 205, 206, 207, 208, rt.G_SPECIAL, rt.G_FINITE)}
    assert s[at[201]] == np.inf and avg[at[201]] == np.inf and mx[at[201]] == np.inf and mn[at[201]] == -3.5
    assert np.isnan(s[at[202]]) and np.isnan(avg[at[202]])                  # inf + -inf
    assert mx[at[202]] == np.inf and mn[at[202]] == -np.inf
    assert np.isnan(s[at[203]]) and cols[4][at[203]] == rt.HIGHEST_NAN and mn[at[203]] == 1.0    # a NaN is the MAX
    assert s[at[204]] == -np.inf and avg[at[204]] == -np.inf
    assert s[at[205]] == 1e-323 and mx[at[205]] == 5e-324 and mn[at[205]] == -5e-324              # subnormals
    assert s[at[206]] == 0.0 and mx[at[206]] == 0.0 and mn[at[206]] == 0.0                        # either sign
    assert cols[2][at[207]] == np.int64(-(1 << 63))                         # -0.0 + -0.0 is -0.0 in any order
    assert np.isnan(s[at[rt.G_SPECIAL]])
    assert cols[4][at[rt.G_SPECIAL]] == rt.HIGHEST_NAN                      # MAX / MIN with NaNs: the image order
    assert cols[5][at[rt.G_SPECIAL]] == np.array([rt.LOWEST_NAN], np.uint64).view(np.int64)[0]
    fin = _by_key([ref.keys[0]], rt.G_FINITE)
    assert ref.count[fin] > 500 and ref.cols[1].tol[fin] > 0                # an inexact sum, held to the derived bound


def test_std_where_the_rule_holds(vg):
    """STD(x) over multiples of 1/8 (every sum exact, so the device's avg is the reference's and
    both add the same non-negative terms) and STD(i) over the same rows."""
    idx = vg.t.rows_of_sources(rt.EXTRA_SRC0 + rt.G_EXACT, rt.EXTRA_SRC0 + rt.G_EXACT + 1)
    assert len(idx) == 40
    rows, _ = rt.go_checked(vg.ld, idx)
    try:
        _group(vg, ["g"], [("COUNT", None), ("STD", "x"), ("STD", "i"), ("AVG", "x"), ("SUM", "x")], rows, idx)
        _group(vg, [], [("COUNT", None), ("STD", "x"), ("STD", "i")], rows, idx)
    finally:
        rows.free()


# ------------------------------------------------------------------------------ 5. COUNT_DISTINCT
@pytest.mark.parametrize("keys", [[], ["b"], ["g"], ["s"]], ids=lambda k: "_".join(k) or "const")
def test_count_distinct(vg, keys):
    aggs = [("COUNT", None), ("COUNT_DISTINCT", "x"), ("COUNT_DISTINCT", "i"), ("COUNT_DISTINCT", "s"),
            ("COUNT_DISTINCT", "z"), ("COUNT_DISTINCT", "d"), ("COUNT_DISTINCT", "b"), ("COUNT_DISTINCT", "t")]
    cols, ref = _group(vg, keys, aggs)
    nk = len(keys)
    assert (cols[nk + 4] == 1).all()                                        # zeros of both signs: one value
    if not keys:
        x = vg.t.bits["x"].view(np.uint64)
        folded = np.where(x == np.uint64(1 << 63), np.uint64(0), x)
        assert cols[1][0] == len(np.unique(folded))                         # zeros one, the NaNs by their bits
        assert len(np.unique(folded)) == len(np.unique(x)) - 1
        assert cols[3][0] == len(rt.STRS) and cols[5][0] == len(rt.VIDS)


# ------------------------------------------------------------------------------ 6. NaN under MAX / MIN
@pytest.mark.parametrize("keys", [[], ["c"], ["b"]], ids=lambda k: "_".join(k) or "const")
def test_nan_max_min_is_the_image_order(vg, keys):
    """The reference's MAX / MIN keep whatever NaN or number came first; the device reduces the
    IEEE total-order images (include/nbg.h), so wherever a group holds them the MAX is the highest
    positive NaN and the MIN the lowest negative one, in any row order: on the GO's segments and on
    the ORDER BY x DESC copy of them."""
    aggs = [("COUNT", None), ("MAX", "x"), ("MIN", "x")]
    lowest = np.array([rt.LOWEST_NAN], np.uint64).view(np.int64)[0]
    x, b = vg.t.bits["x"].view(np.float64), vg.t.bits["b"]
    for side in (0, 1):                                  # both BOOL groups hold NaNs of both signs
        assert (np.isnan(x) & ~np.signbit(x) & (b == side)).any() and (np.isnan(x) & np.signbit(x) & (b == side)).any()
    ordered = vg.ld.eng.order_by(vg.rows, vg.ld.names, [("x", True)])
    try:
        for inp in (vg.rows, ordered):
            cols, _ = _group(vg, keys, aggs, inp)        # (group_ref reduces the images: the rule itself)
            nk = len(keys)
            mx, mn = cols[nk + 1].view(np.float64), cols[nk + 2].view(np.float64)
            assert np.isnan(mx).all() and not np.signbit(mx).any() and np.isnan(mn).all() and np.signbit(mn).all()
            if keys != ["b"]:                            # one group: the table's highest and lowest NaN
                assert cols[nk + 1][0] == rt.HIGHEST_NAN and cols[nk + 2][0] == lowest
    finally:
        ordered.free()
