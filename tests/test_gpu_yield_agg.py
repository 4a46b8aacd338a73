"""nbg_yield_agg on the MI355X: the piped YIELD with aggregate functions and no GROUP BY over
device-resident rows.  Expected values come from numpy / Python over the cells of rowtable tables
(tests/support/rowtable.py) and from the reference's own YieldTest.AggCall vectors
(tests/golden/yield_golden.json) — never from the device.

Typing is include/nbg.h's for this call, not nbg_group_by's: a bare column reads as its kind's own
type, so the VID column d and the TIMESTAMP column t are INT here (AVG, STD and BIT_* are defined
over them) and the only TIMESTAMP-typed argument is a root `(timestamp)' cast.  With no row kept the
result is each fresh function object's getResult.  `_expect` below restates those rules.

Comparison: ints, counts, MAX / MIN, BIT_* and the integer AVG by bits; a double SUM against
math.fsum within gamma_{n-1} * sum|x_i| (rowtable.sum_ref), a double AVG within that bound over n
plus the quotient's rounding; STD within relative n * 2^-52, on arguments whose mean is exact (ints,
multiples of 1/8); a sum with a NaN or infinities among its terms by class and sign.

Three NBG_E_UNSUPPORTED cases of include/nbg.h have no test because no GO result reaches them: a
column whose kind differs between OVER types, MAX / MIN / COUNT_DISTINCT over a string expression
that builds no string, and the input of 2^32 rows."""
import math

import numpy as np
import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E
from nebula_amd.engine import nba_engine
from tests.support import golden, ngql, rowtable as rt, yieldpipe
from tests.support.setops import Value
from tests.test_gpu_orderby import E_SCHEMA, GO_COLS, PARTS, ROOTS, T_SCHEMA, _kv

pytestmark = pytest.mark.gpu

GOLDEN = golden.load("yield_golden.json")["cases"]
OB_CHUNK, STAGE_GRID, BLOCK = 2048, 2048, 256          # csrc/nbg_internal.h, csrc/stage.h, csrc/ws.h
EMPTY_SRC = 123
FUNS = ["COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MAX", "MIN", "STD", "BIT_AND", "BIT_OR", "BIT_XOR"]
TS = "timestamp"                                       # the type of a root (timestamp) cast
NAN_BITS = 0x7FF8000000000000


class Fixture:
    pass


def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


def _args(text):
    st = yieldpipe.parse_sentence(text)
    return ([c.expr.encode() for c in st.yields], [c.fun if c.fun else 0 for c in st.yields],
            st.where.encode() if st.where is not None else b"")


def _agg(eng, rows, names, text):
    ys, funs, where = _args(text)
    return eng.yield_agg(rows, names, ys, funs, where)


def _one_row(eng, out):
    """(bits per column, kinds) of a one-row result; the result is freed."""
    try:
        assert out.count == 1 and eng.lib.nbg_rows_num_segments(out.h) == 1
        kinds = [eng.lib.nbg_rows_col_kind(out.h, c) for c in range(eng.lib.nbg_rows_num_cols(out.h))]
        return [int(c[0]) for c in out.fetch_bits()], kinds
    finally:
        out.free()


# ------------------------------------------------------------------------------ the expectation
class Exp:
    def __init__(self, kind, bits, how="exact", tol=0.0):
        self.kind, self.bits, self.how, self.tol = kind, int(bits) & ((1 << 64) - 1), how, tol


def _expect(fun, bits, typ):
    """The result cell of `fun` over the kept argument cells `bits` (int64 payloads) of type `typ`
    (rt.INT, rt.DOUBLE, rt.BOOL, rt.STRING as ranks, or TS), as include/nbg.h states it."""
    n = len(bits)
    dbl0, nan = Exp(L.V_DOUBLE, rt.dbits(0.0)), Exp(L.V_DOUBLE, NAN_BITS, "nan")
    if fun == "COUNT":
        return Exp(L.V_INT, n)
    if fun == "COUNT_DISTINCT":
        return Exp(L.V_INT, len(np.unique(rt.fold_zero(bits, typ))))
    if n == 0:                                          # a fresh function object's getResult
        assert fun not in ("MAX", "MIN"), "status 9"
        return nan if fun == "AVG" else Exp(L.V_INT, 0)
    ints = typ in (rt.INT, TS)
    if fun in ("SUM", "AVG"):
        if ints:
            s = int(np.add.reduce(bits.view(np.uint64)).view(np.int64)) if n else 0       # wraps
            if fun == "SUM":
                return Exp(L.V_INT, s)
            assert typ == rt.INT, "AVG over a TIMESTAMP-typed argument is a device limit"
            return Exp(L.V_DOUBLE, rt.dbits(float(np.float64(s) / np.float64(n))))
        if typ != rt.DOUBLE:
            return Exp(L.V_INT, 0) if fun == "SUM" else dbl0
        s, tol = rt.sum_ref(bits.view(np.float64).tolist())
        if fun == "AVG":
            s, tol = s / n, tol / n
            tol = tol + 2 * rt.U * (abs(s) + tol) + 5e-324 if math.isfinite(s) else tol
        return Exp(L.V_DOUBLE, rt.dbits(s), "abs", tol)
    if fun in ("MAX", "MIN"):
        t = rt.INT if typ == TS else typ
        k = rt.order_key(bits, t)
        r = np.array([k.max() if fun == "MAX" else k.min()], np.uint64)
        return Exp(rt.KIND[t], rt.order_unkey(r, t)[0], "zero" if typ == rt.DOUBLE else "exact")
    if fun == "STD":
        if typ not in (rt.INT, rt.DOUBLE):
            return Exp(L.V_INT, 0)
        if typ == rt.INT:
            x = bits.astype(np.float64)
            avg = np.float64(np.add.reduce(bits.view(np.uint64)).view(np.int64)) / np.float64(n)
        else:
            x = bits.view(np.float64)
            avg = np.float64(rt.sum_ref(x.tolist())[0]) / np.float64(n)
        with np.errstate(invalid="ignore", over="ignore"):
            d = x - avg
            std = float(np.sqrt(np.add.reduce(d * d) / n))
        return Exp(L.V_DOUBLE, rt.dbits(std), "rel", n * 2.0 ** -52)
    if typ != rt.INT:
        return Exp(L.V_INT, 0)
    op = {"BIT_AND": np.bitwise_and, "BIT_OR": np.bitwise_or, "BIT_XOR": np.bitwise_xor}[fun]
    return Exp(L.V_INT, op.reduce(bits))


def _check(got_bits, got_kind, exp: Exp, what):
    got_bits &= (1 << 64) - 1
    assert got_kind == exp.kind, (what, "kind", got_kind, exp.kind)
    g, w = rt.dval(got_bits), rt.dval(exp.bits)
    print(f"{what}: device {got_bits:#018x} expected {exp.bits:#018x} ({exp.how}, tol {exp.tol})")
    if exp.how == "exact":
        assert got_bits == exp.bits, what
    elif exp.how == "zero":
        assert got_bits == exp.bits or (g == 0.0 and w == 0.0), what
    elif exp.how == "nan" or math.isnan(w):
        assert math.isnan(g), what
    elif math.isinf(w):
        assert g == w, what
    else:
        bound = exp.tol * (abs(w) if exp.how == "rel" else 1.0)
        assert math.isfinite(g) and abs(g - w) <= bound, (what, g, w, bound)


# ------------------------------------------------------------------------------ golden
class AggSession(yieldpipe.Session):
    """yieldpipe.Session whose device mode sends a YIELD with a function to Engine.yield_agg."""

    def __init__(self, backend, device=False):
        super().__init__(backend, device)
        self.agg_calls = 0

    def execute(self, text):
        self.agg_calls = 0
        return super().execute(text)

    def _stage_device(self, sents, i, src):
        st = sents[i]
        if not (isinstance(st, yieldpipe.YieldSentence) and any(c.fun for c in st.yields)):
            return super()._stage_device(sents, i, src)
        try:
            out = self.b.yield_agg(src.rows, src.names, [c.expr.encode() for c in st.yields],
                                   [c.fun if c.fun else 0 for c in st.yields],
                                   st.where.encode() if st.where is not None else b"")
        except NbgError as ex:
            if ex.code != L.E_UNSUPPORTED:
                raise
            self.fallbacks.append((type(st).__name__, ex.code))
            return self._stage_host(st, src), 1
        self.agg_calls += 1
        return Value([c.name() for c in yieldpipe.expand(st.yields, src.names)], None, rows=out), 1


def _is_agg_over_input(case):
    return case["test"] == "AggCall" and case["status"] == "SUCCEEDED" and ("$-." in case["query"] or "$var." in case["query"])


@pytest.fixture(scope="module")
def nba(nba_data):
    eng = nba_engine(nba_data)
    yield eng
    eng.close()


def test_golden_aggregate_cases_stay_on_the_device(nba):
    cases = [c for c in GOLDEN if _is_agg_over_input(c)]
    assert len(cases) == 2 and any("$var." in c["query"] for c in cases)
    assert sorted(c["expected"][0] for c in cases) == [[34.666666666666664, 270, 3], [34.666666666666664, 270, 3, 2]]
    for case in cases:
        ses = AggSession(nba, device=True)
        ok, msg = yieldpipe.run_case(ses, case)
        assert ok, msg
        assert not ses.fallbacks and ses.agg_calls == 1 and ses.yield_calls == 0


@pytest.mark.parametrize("case", [c for c in GOLDEN if c["test"] == "AggCall"],
                         ids=[f"AggCall-{i}" for i, c in enumerate(GOLDEN) if c["test"] == "AggCall"])
def test_golden_agg_call_cases(nba, case):
    """Every AggCall vector, the failing ones (checkAggFun) and the constant ones included."""
    ok, msg = yieldpipe.run_case(AggSession(nba, device=True), case)
    assert ok, msg


# ------------------------------------------------------------------------------ the value table
@pytest.fixture(scope="module")
def vt():
    f = Fixture()
    f.t = rt.value_table()
    f.ld = rt.load_value_table(f.t)
    f.rows, _ = rt.go_checked(f.ld)
    f.names = f.ld.names
    f.one = f.ld.by_pos(f.rows)
    assert f.ld.eng.lib.nbg_rows_num_segments(f.rows.h) >= 2 and f.ld.eng.lib.nbg_rows_num_segments(f.one.h) == 1
    f.digest = f.rows.digest()
    yield f
    f.rows.free()
    f.one.free()
    f.ld.close()


COL_TYPE = {"i": rt.INT, "d": rt.INT, "t": rt.INT, "x": rt.DOUBLE, "s": rt.STRING, "b": rt.BOOL}
WHERE_TEXT = "$-.pos % 3 != 1"


def _keep(t, where):
    pos = t.bits["pos"]
    return {None: pos >= 0, WHERE_TEXT: pos % 3 != 1, "finite": (t.bits["g"] >= 300) & (t.bits["g"] < 310),
            "exact": t.bits["g"] == rt.G_EXACT}[where]


WHERES = {None: "", WHERE_TEXT: " WHERE " + WHERE_TEXT, "finite": " WHERE $-.g >= 300 && $-.g < 310",
          "exact": f" WHERE $-.g == {rt.G_EXACT}"}


def _run_funs(vt, arg_text, arg_bits, typ, where, funs=FUNS, string=False):
    """Every function of `funs` over one argument, in one call, over the raw GO result and over its
    one-segment copy, against _expect over the table's cells."""
    keep = _keep(vt.t, where)
    text = "YIELD " + ", ".join(f"{f}({arg_text})" for f in funs) + WHERES[where]
    exps = [_expect(f, arg_bits[keep], typ) for f in funs]
    eng = vt.ld.eng
    for rows in (vt.rows, vt.one):
        out = _agg(eng, rows, vt.names, text)
        if string:                                     # MAX / MIN of the string column: codes to the table's ranks
            names = [f"c{k}" for k in range(len(funs))]
            cols = vt.ld.bits_of(out, names, [n for n, f in zip(names, funs) if f in ("MAX", "MIN")])
            kinds = vt.ld.kinds_of(out)
            got = [int(cols[n][0]) for n in names]
            out.free()
        else:
            got, kinds = _one_row(eng, out)
        for f, g, k, e in zip(funs, got, kinds, exps):
            _check(g, k, e, f"{f}({arg_text}){WHERES[where]} [{'raw' if rows is vt.rows else 'one'}]")


@pytest.mark.parametrize("where", [None, WHERE_TEXT])
@pytest.mark.parametrize("col", list(COL_TYPE))
def test_bare_columns(vt, col, where):
    """Every function over a bare column of every type.  d (VID) and t (TIMESTAMP) are INT here."""
    _run_funs(vt, f"$-.{col}", vt.t.bits[col], COL_TYPE[col], where, string=col == "s")


def test_bare_columns_agree_with_group_ref(vt):
    """Where GroupByExecutor's typing agrees (INT, DOUBLE, BOOL columns), rowtable.group_ref over no
    keys is the same reference."""
    keep = np.nonzero(_keep(vt.t, WHERE_TEXT))[0]
    for col in ("i", "b"):
        ref = rt.group_ref(vt.t, [], [(f, col) for f in FUNS], keep)
        for f, rc in zip(FUNS, ref.cols):
            e = _expect(f, vt.t.bits[col][keep], COL_TYPE[col])
            if rc.how == "exact":
                assert (int(rc.bits[0]) & ((1 << 64) - 1)) == e.bits and rc.kind == e.kind, (col, f)


def test_double_std_and_sums_on_exact_inputs(vt):
    """x over the rows whose cells are multiples of 1/8: the mean is exact."""
    _run_funs(vt, "$-.x", vt.t.bits["x"], rt.DOUBLE, "exact")
    _run_funs(vt, "$-.x", vt.t.bits["x"], rt.DOUBLE, "finite", [f for f in FUNS if f != "STD"])


@pytest.mark.parametrize("where", [None, WHERE_TEXT])
def test_expressions(vt, where):
    t = vt.t
    with np.errstate(over="ignore"):
        _run_funs(vt, "$-.i * 3 + $-.g", t.bits["i"] * 3 + t.bits["g"], rt.INT, where)
    _run_funs(vt, "(double)$-.i", t.bits["i"].astype(np.float64).view(np.int64), rt.DOUBLE, where)
    _run_funs(vt, "(timestamp)$-.i", t.bits["i"], TS, where, ["SUM", "MAX", "MIN", "STD", "COUNT", "BIT_OR", "COUNT_DISTINCT"])
    x = t.bits["x"].view(np.float64)
    with np.errstate(invalid="ignore"):
        _run_funs(vt, "$-.x < 0.0", (x < 0.0).astype(np.int64), rt.BOOL, where)
    # x * 0.5: arithmetic over a NaN leaves its payload to the implementation, so every function over
    # the finite rows, and over all rows what does not depend on a NaN's bits
    with np.errstate(invalid="ignore"):
        half = (x * 0.5).view(np.int64)
    _run_funs(vt, "$-.x * 0.5", half, rt.DOUBLE, "finite", [f for f in FUNS if f != "STD"])
    _run_funs(vt, "$-.x * 0.5", half, rt.DOUBLE, where, ["COUNT", "SUM", "AVG", "BIT_AND"])


def test_count_star_constants_and_shared_arguments(vt):
    t, eng = vt.t, vt.ld.eng
    keep = _keep(t, WHERE_TEXT)
    n = int(keep.sum())
    text = ('YIELD COUNT(*), 1+1, SUM(5), AVG(2.5), MAX("abc"), MIN(7), COUNT_DISTINCT(*), COUNT_DISTINCT(3), STD(4), '
            'BIT_OR(6), SUM("x"), COUNT($-.x)' + WHERES[WHERE_TEXT])
    for rows in (vt.rows, vt.one):
        out = _agg(eng, rows, vt.names, text)
        assert out.fetch() == [[n, 2, 5 * n, 2.5, "abc", 7, 1, 1, 0.0, 6, 0, n]]
        out.free()
    # AVG(e), SUM(e), STD(e): one sum.  The slots are shared, so the 10 functions twice over fit too.
    e = "$-.i % 1000 + $-.g"
    i, g = t.bits["i"], t.bits["g"]
    arg = (np.fmod(i, 1000) + g)                        # C++ % truncates toward zero
    _run_funs(vt, e, arg, rt.INT, WHERE_TEXT, ["AVG", "SUM", "STD", "SUM", "AVG", "STD"] + FUNS)
    eng.profile(True)
    _agg(eng, vt.rows, vt.names, f"YIELD AVG({e}), SUM({e}), STD({e}), COUNT(*)").free()
    prof = eng.profile_read()
    eng.profile(False)
    assert prof["k_ya_reduce"]["launches"] == 2 and prof["k_ya_finish"]["launches"] == 2     # the sums, then the squares
    # partials: 8 bytes per slot and 4 per chunk; two slots (one sum, one square) for the three columns
    nchunks = sum(-(-m // OB_CHUNK) for _, m in vt.ld.segments(vt.rows))
    assert prof["k_ya_finish"]["algo_bytes"] == 2 * nchunks * (8 * 2 + 4)


# ------------------------------------------------------------------------------ row counts
ROW_COUNTS = [1, 255, 256, 257, 2047, 2048, 2049]
SRC_SIZES = np.diff([0] + ROW_COUNTS)


@pytest.fixture(scope="module")
def ct():
    """v (INT, random) and y (DOUBLE: multiples of 1/16 whose sums are exact in any order); the
    first k + 1 sources hold ROW_COUNTS[k] rows."""
    rng = np.random.default_rng(91)
    n = ROW_COUNTS[-1]
    f = Fixture()
    f.t = rt.Table([("v", rt.INT, rng.integers(-(1 << 40), 1 << 40, n)),
                    ("y", rt.DOUBLE, (rng.integers(-(1 << 30), 1 << 30, n) / 16.0).view(np.uint64))],
                   src=np.repeat(np.arange(len(SRC_SIZES)), SRC_SIZES))
    f.ld = rt.load_numeric_table(f.t)
    f.names = f.ld.names
    yield f
    f.ld.close()


COUNT_TEXT = "YIELD COUNT(*), SUM($-.v * 2 + 1), MAX($-.v), MIN($-.y), SUM($-.y), BIT_XOR($-.v), STD($-.v), AVG($-.y)"
COUNT_SPEC = [("COUNT", None), ("SUM", "w"), ("MAX", "v"), ("MIN", "y"), ("SUM", "y"), ("BIT_XOR", "v"), ("STD", "v"), ("AVG", "y")]


def _count_case(ct, rows, where_text, keep, what):
    t = ct.t
    cells = {"v": t.bits["v"], "y": t.bits["y"], "w": t.bits["v"] * 2 + 1, None: t.bits["pos"]}
    types = {"v": rt.INT, "w": rt.INT, "y": rt.DOUBLE, None: rt.INT}
    got, kinds = _one_row(ct.ld.eng, _agg(ct.ld.eng, rows, ct.names, COUNT_TEXT + (" WHERE " + where_text if where_text else "")))
    for (f, c), g, k in zip(COUNT_SPEC, got, kinds):
        e = _expect(f, cells[c][keep], types[c])
        if c == "y":
            e.how, e.tol = ("zero" if f == "SUM" else e.how), (0.0 if f == "SUM" else e.tol)   # these sums are exact
        _check(g, k, e, f"{what}: {f}({c})")


@pytest.mark.parametrize("k", range(len(ROW_COUNTS)), ids=[f"rows{c}" for c in ROW_COUNTS])
def test_input_row_counts(ct, k):
    n = ROW_COUNTS[k]
    raw = ct.ld.go([rt.SRC0 + s for s in range(k + 1)])
    one = ct.ld.by_pos(raw)
    try:
        assert raw.count == n == one.count
        member = ct.t.bits["pos"] < n
        last = min(n, OB_CHUNK) - 1
        for rows in (raw, one):
            for where, keep in ((None, member), ("$-.pos == 0", ct.t.bits["pos"] == 0),
                                (f"$-.pos == {last}", ct.t.bits["pos"] == last),            # the last row of a chunk
                                (f"$-.pos == {n - 1}", ct.t.bits["pos"] == n - 1),
                                ("$-.pos % 2 == 1", member & (ct.t.bits["pos"] % 2 == 1))):
                if keep.any():
                    _count_case(ct, rows, where, keep, f"{n} rows, WHERE {where}")
    finally:
        raw.free()
        one.free()


def test_kept_row_counts(ct):
    """Kept counts at every edge over the 2,049-row input, and a WHERE that keeps nothing in the
    whole first chunk."""
    raw = ct.ld.go()
    one = ct.ld.by_pos(raw)
    pos = ct.t.bits["pos"]
    try:
        for rows in (raw, one):
            for kept in ROW_COUNTS:
                _count_case(ct, rows, f"$-.pos < {kept}", pos < kept, f"{kept} kept")
            _count_case(ct, rows, f"$-.pos >= {OB_CHUNK}", pos >= OB_CHUNK, "only the last chunk's row")
            _count_case(ct, rows, f"$-.pos >= {OB_CHUNK - 1}", pos >= OB_CHUNK - 1, "a chunk's last row and the next's first")
    finally:
        raw.free()
        one.free()


# ------------------------------------------------------------------------------ identities
ALL_ONES, MAX_IMAGE = 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF


def test_a_kept_value_equal_to_the_identity(ct):
    """Whether a row was kept decides what enters an accumulator, never its value."""
    rng = np.random.default_rng(3)
    n = 700
    v = rng.integers(-1000, 1000, n)
    y = rng.integers(-1000, 1000, n).astype(np.float64).view(np.uint64)
    v[:4] = [rt.INT64_MIN, rt.INT64_MAX, -1, 0]
    y[:4] = [1 << 63, ALL_ONES, MAX_IMAGE, rt.dbits(1.0)]
    t = rt.Table([("v", rt.INT, v), ("y", rt.DOUBLE, y)], per_src=100)
    ld = rt.load_numeric_table(t)
    raw, _ = rt.go_checked(ld)
    one = ld.by_pos(raw)
    u64 = (1 << 64) - 1
    cases = [(0, "MAX($-.v)", rt.INT64_MIN & u64), (1, "MIN($-.v)", rt.INT64_MAX), (2, "BIT_AND($-.v)", u64),
             (3, "SUM($-.v)", 0), (3, "BIT_OR($-.v)", 0), (3, "BIT_XOR($-.v)", 0), (0, "SUM($-.y)", 1 << 63),
             (1, "MAX($-.y)", ALL_ONES), (2, "MIN($-.y)", MAX_IMAGE)]
    try:
        for rows in (raw, one):
            for pos, fun, want in cases:
                got, _ = _one_row(ld.eng, _agg(ld.eng, rows, ld.names, f"YIELD {fun}, COUNT(*) WHERE $-.pos == {pos}"))
                assert (got[0] & u64, got[1]) == (want, 1), (fun, hex(got[0] & u64))
    finally:
        raw.free()
        one.free()
        ld.close()


# ------------------------------------------------------------------------------ no kept rows
NONE_TEXT = "YIELD COUNT(*), COUNT_DISTINCT($-.i), SUM($-.x), AVG($-.i), STD($-.x), BIT_OR($-.i)"


def test_no_kept_rows(vt):
    eng = vt.ld.eng
    for where in (" WHERE $-.pos < 0", " WHERE 1 > 2"):         # on the device, and folded to a constant
        for rows in (vt.rows, vt.one):
            got, kinds = _one_row(eng, _agg(eng, rows, vt.names, NONE_TEXT + where))
            assert kinds == [L.V_INT, L.V_INT, L.V_INT, L.V_DOUBLE, L.V_INT, L.V_INT]      # SUM of a double: INT 0
            assert got[:3] == [0, 0, 0] and math.isnan(rt.dval(got[3])) and got[4:] == [0, 0]
            assert _code(lambda: _agg(eng, rows, vt.names, NONE_TEXT.replace("YIELD", "YIELD MAX($-.i),") + where)) == L.E_EXECUTION_ERROR
            assert _code(lambda: _agg(eng, rows, vt.names, NONE_TEXT + ", 1+1" + where)) == L.E_EXECUTION_ERROR
    with pytest.raises(NbgError, match="Not Support: 0"):
        _agg(eng, vt.rows, vt.names, "YIELD MIN($-.x) WHERE $-.pos < 0")
    empty = vt.ld.go([EMPTY_SRC])
    try:
        assert empty.count == 0
        out = _agg(eng, empty, vt.names, NONE_TEXT + ", MAX($-.i), 1+1")
        assert out.count == 0 and eng.lib.nbg_rows_num_cols(out.h) == 8 and out.fetch() == []
        out.free()
    finally:
        empty.free()


# ------------------------------------------------------------------------------ statuses, in nbg.h's order
@pytest.fixture(scope="module")
def gf():
    """tests/test_gpu_orderby.py's graph: k7, d, s (dictionary strings), w, x, z, b2."""
    _, kb = _kv()
    f = Fixture()
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_tag(7, "t", T_SCHEMA)
    f.eng.load_builder(kb)
    sent = ngql.Parser(f"GO 2 STEPS FROM 1 OVER e YIELD {GO_COLS}").go()
    f.names = [c.name() for c in sent.yields]
    f.rows = f.eng.go_device(ROOTS, [1], 2, b"", [c.expr.encode() for c in sent.yields])
    f.inp = f.rows.fetch()
    f.w = np.array([r[f.names.index("w")] for r in f.inp], np.int64)
    yield f
    f.rows.free()
    f.eng.close()


def _go(eng, yields, root=ROOTS[0], steps=1):
    sent = ngql.Parser(f"GO FROM 1 OVER e YIELD {yields}").go()
    return eng.go_device([root], [1], steps, b"", [c.expr.encode() for c in sent.yields]), [c.name() for c in sent.yields]


def test_status_1_invalid_arguments(gf):
    eng, rows, names = gf.eng, gf.rows, gf.names
    w = E.input_prop("w").encode()
    assert _code(lambda: eng.yield_agg(rows, names, [], [])) == L.E_INVALID_ARGUMENT
    assert _code(lambda: eng.yield_agg(rows, names, [w], None)) == L.E_INVALID_ARGUMENT            # a null yield_funs
    assert _code(lambda: eng.yield_agg(rows, names, [w, E.const(1).encode()], [0, 0])) == L.E_INVALID_ARGUMENT   # nbg_yield's request
    for bad in (-1, 11):
        assert _code(lambda: eng.yield_agg(rows, names, [w], [bad])) == L.E_INVALID_ARGUMENT
    assert _code(lambda: eng.yield_agg(rows, names, [b"\xff"], ["SUM"])) == L.E_INVALID_ARGUMENT
    assert _code(lambda: eng.yield_agg(rows, names, [w], ["SUM"], b"\xff")) == L.E_INVALID_ARGUMENT
    # ... before the syntax check of another column
    assert _code(lambda: eng.yield_agg(rows, names, [E.edge_prop("e", "w").encode(), b"\xff"], ["SUM", "SUM"])) == L.E_INVALID_ARGUMENT
    # nbg_yield keeps refusing the request
    assert _code(lambda: eng.yield_rows(rows, names, [w], b"", ["SUM"])) == L.E_UNSUPPORTED


def test_status_2_partitioned_engine():
    _, kb = _kv()
    c = LocalCluster(PARTS, 2)
    try:
        c.register_edge(1, "e", E_SCHEMA)
        c.register_tag(7, "t", T_SCHEMA)
        c.load_builder(kb)
        ys = [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "w").encode()]
        rows = c.each(lambda e: e.go_device([ROOTS[0]], [1], 1, b"", ys))
        for e, r in zip(c.engines, rows):
            assert _code(lambda: _agg(e, r, ["d", "w"], "YIELD SUM($-.w)")) == L.E_UNSUPPORTED
            assert _code(lambda: _agg(e, r, ["d", "w"], "YIELD SUM(e.w), $-.d")) == L.E_UNSUPPORTED       # before 3
            r.free()
    finally:
        c.close()


def test_statuses_3_to_6_in_order(gf):
    eng, rows, names = gf.eng, gf.rows, gf.names
    empty, enames = _go(eng, "e._dst AS d, e.w AS w", EMPTY_SRC)
    try:
        # 3: syntaxCheck and checkAggFun, before 4, 5 and 6
        for text in ("YIELD SUM($^.t.name)", "YIELD COUNT(*), e.w", "YIELD COUNT(*) WHERE $$.t.name == \"n1\"",
                     "YIELD COUNT(*), $-.d", "YIELD SUM($-.w), $v.d", "YIELD SUM($-.zz), $-.d", "YIELD MAX($-.*), $-.*"):
            assert _code(lambda: _agg(eng, rows, names, text)) == L.E_SYNTAX_ERROR, text
        assert _code(lambda: _agg(eng, empty, enames, "YIELD COUNT(*), $-.d")) == L.E_SYNTAX_ERROR
        with pytest.raises(NbgError, match="Input columns without aggregation are not supported in YIELD statement"):
            _agg(eng, rows, names, "YIELD COUNT(*), $-.w")
        # 4, before 5 and 6
        for text in ("YIELD SUM($-.w), MAX($v.w)", "YIELD SUM($v.w) WHERE $u.zz > 1"):
            assert _code(lambda: _agg(eng, rows, names, text)) == L.E_EXECUTION_ERROR
            assert _code(lambda: _agg(eng, empty, enames, text)) == L.E_EXECUTION_ERROR
        # 5, before 6 and 7
        for text, ncols in (("YIELD SUM($-.zz), COUNT(*)", 2), ("YIELD MAX($-.*), 1+1", 3), ('YIELD COUNT($-.w + "x")', 1)):
            out = _agg(eng, empty, enames, text)
            assert out.count == 0 and eng.lib.nbg_rows_num_cols(out.h) == ncols
            out.free()
        # 6, before 7: an unknown column beside a string-building column, beside AVG of a timestamp
        with pytest.raises(NbgError, match="column `zz' not exist in input.") as ex:
            _agg(eng, rows, names, 'YIELD SUM($-.zz), COUNT($-.s + "x")')
        assert ex.value.code == L.E_EXECUTION_ERROR
        with pytest.raises(NbgError, match="column `zz' not exist in variable."):
            _agg(eng, rows, names, "YIELD AVG((timestamp)$v.w) WHERE $v.zz > 0")
        dup = ["a", "a"] + names[2:]                    # the first match wins
        got, _ = _one_row(eng, _agg(eng, rows, dup, "YIELD SUM($-.a)"))
        assert got[0] == sum(r[0] for r in gf.inp)
    finally:
        empty.free()


def test_status_8_evaluation_errors(gf):
    """`$-.w / ($-.w + 7)` fails on the rows with w == -7."""
    eng, rows, names, w = gf.eng, gf.rows, gf.names, gf.w
    assert (w == -7).any()
    digest = rows.digest()
    q = "$-.w / ($-.w + 7)"
    assert _code(lambda: _agg(eng, rows, names, f"YIELD SUM({q})")) == L.E_EXECUTION_ERROR             # an argument, a kept row
    assert _code(lambda: _agg(eng, rows, names, f"YIELD COUNT({q}) WHERE $-.w < 0")) == L.E_EXECUTION_ERROR
    assert _code(lambda: _agg(eng, rows, names, f"YIELD COUNT(*) WHERE {q} > 0")) == L.E_EXECUTION_ERROR   # the WHERE, any row
    assert _code(lambda: _agg(eng, rows, names, f"YIELD COUNT_DISTINCT({q})")) == L.E_EXECUTION_ERROR
    assert _code(lambda: _agg(eng, rows, names, "YIELD COUNT(*), 1/0")) == L.E_EXECUTION_ERROR
    assert _code(lambda: _agg(eng, rows, names, "YIELD SUM($-.b2 + 1)")) == L.E_EXECUTION_ERROR        # ill-typed: every row
    keep = w != -7                                                                                      # a rejected row: no error
    quot = np.trunc(w[keep] / (w[keep] + 7.0)).astype(np.int64)
    got, _ = _one_row(eng, _agg(eng, rows, names, f"YIELD SUM({q}), COUNT(*), COUNT_DISTINCT({q}) WHERE $-.w != -7"))
    assert got == [int(quot.sum()), int(keep.sum()), len(np.unique(quot))]
    assert rows.digest() == digest


# ------------------------------------------------------------------------------ device limits
@pytest.mark.parametrize("text", ["YIELD COUNT(*), $-.w + 1", "YIELD SUM($-.w), rand32()", "YIELD SUM($-.w), now()"])
def test_limit_a_column_without_a_function_that_is_not_constant(gf, text):
    assert _code(lambda: _agg(gf.eng, gf.rows, gf.names, text)) == L.E_UNSUPPORTED


def test_limit_avg_of_a_timestamp(gf):
    assert _code(lambda: _agg(gf.eng, gf.rows, gf.names, "YIELD AVG((timestamp)$-.w)")) == L.E_UNSUPPORTED
    got, _ = _one_row(gf.eng, _agg(gf.eng, gf.rows, gf.names, "YIELD SUM((timestamp)$-.w), STD((timestamp)$-.w)"))
    assert got == [int(gf.w.sum()), 0]


@pytest.mark.parametrize("text", ['YIELD COUNT($-.s + "!")', "YIELD MAX((string)$-.w)", "YIELD COUNT_DISTINCT(upper($-.s))",
                                  "YIELD SUM($-.w), MIN(lpad(left($-.s, 2), 5, $-.s)) WHERE $-.w > 0"])
def test_limit_string_building(gf, text):
    """An argument that stores a string it built (the programs with OP_SOUT / OP_SMAT).  A WHERE that
    only compares such a string stores none and is answered."""
    assert _code(lambda: _agg(gf.eng, gf.rows, gf.names, text)) == L.E_UNSUPPORTED
    got, _ = _one_row(gf.eng, _agg(gf.eng, gf.rows, gf.names, 'YIELD COUNT(*), SUM($-.w) WHERE (string)$-.w == "-7"'))
    assert got == [int((gf.w == -7).sum()), -7 * int((gf.w == -7).sum())]


def test_limit_strings_outside_the_dictionary(gf):
    for ys in ('$$.t.name + "!" AS s, e.w AS w', '"no such name" AS s, e.w AS w'):
        rows, names = _go(gf.eng, ys, ROOTS[0], 2)
        try:
            n = rows.count
            for text in ("YIELD MAX($-.s)", "YIELD MIN($-.s)", "YIELD COUNT_DISTINCT($-.s)", 'YIELD COUNT(*) WHERE $-.s < "n1"',
                         "YIELD SUM(hash($-.s))"):
                assert _code(lambda: _agg(gf.eng, rows, names, text)) == L.E_UNSUPPORTED, text
            got, _ = _one_row(gf.eng, _agg(gf.eng, rows, names, "YIELD COUNT($-.s), SUM($-.s), BIT_OR($-.s)"))
            assert got == [n, 0, 0]
        finally:
            rows.free()
    got = _agg(gf.eng, gf.rows, gf.names, "YIELD MAX($-.s), MIN($-.s), COUNT_DISTINCT($-.s)")      # inside the dictionary
    s = [r[gf.names.index("s")].encode() for r in gf.inp]
    assert got.fetch() == [[max(s).decode(), min(s).decode(), len(set(s))]]
    got.free()


def test_limit_float_and_misaligned_inputs(gf):
    for ys in ("e._dst AS d, e.f AS f", "e._dst AS d, e.x + e.w AS m, e.w AS w"):
        rows, names = _go(gf.eng, ys)
        try:
            assert _code(lambda: _agg(gf.eng, rows, names, "YIELD MAX($-.d)")) == L.E_UNSUPPORTED
        finally:
            rows.free()


def test_limit_columns_program_and_registers(gf):
    rows, names = _go(gf.eng, ", ".join(f"e.w + {k} AS c{k}" for k in range(17)), ROOTS[0])
    try:
        star = E.input_prop("*").encode()
        assert _code(lambda: gf.eng.yield_agg(rows, names, [star, star], ["MAX", "MIN"])) == L.E_UNSUPPORTED      # 34 columns
        w = np.array([r[0] for r in rows.fetch()], np.int64)
        got, _ = _one_row(gf.eng, gf.eng.yield_agg(rows, names, [star, E.const("*").encode()], ["SUM", "COUNT"]))
        assert got == [int((w + k).sum()) for k in range(17)] + [len(w)]
        terms = [f"$-.c0 * {k}" for k in range(100)]
        while len(terms) > 1:
            terms = [f"({a} + {b})" if b else a for a, b in zip(terms[0::2], terms[1::2] + [None])]
        assert _code(lambda: _agg(gf.eng, rows, names, f"YIELD SUM({terms[0]})")) == L.E_UNSUPPORTED              # > 256 instructions
        # 32 STDs over 32 different arguments: 64 accumulator slots, past any register file
        with pytest.raises(NbgError, match="register") as ex:
            _agg(gf.eng, rows, names, "YIELD " + ", ".join(f"STD($-.c0 + {k})" for k in range(32)))
        assert ex.value.code == L.E_UNSUPPORTED
    finally:
        rows.free()


# ------------------------------------------------------------------------------ repeatability and hygiene
def test_repeatable_and_feeds_every_stage(vt):
    eng = vt.ld.eng
    text = "YIELD SUM($-.x) AS a, AVG($-.x * 0.5) AS b, STD((double)$-.i) AS c, COUNT(*) AS n, MAX($-.i) AS m WHERE $-.g >= 300 && $-.g < 310"
    a, b = _agg(eng, vt.rows, vt.names, text), _agg(eng, vt.rows, vt.names, text)
    other = _agg(eng, vt.rows, vt.names, text.replace("310", "302"))
    try:
        assert a.digest() == b.digest() and a.fetch_bits()[0][0] == b.fetch_bits()[0][0]
        assert vt.rows.digest() == vt.digest
        names = ["a", "b", "c", "n", "m"]
        row = a.fetch()[0]
        ys, _, where = _args("YIELD $-.n + 1, $-.a WHERE $-.n > 0")
        out = eng.yield_rows(a, names, ys, where)
        assert out.fetch() == [[row[3] + 1, row[0]]]
        out.free()
        both = eng.set_op(a, other, "UNION", distinct=False)
        assert both.count == 2 and both.fetch() == [row, other.fetch()[0]]
        top = eng.order_by(both, names, [("n", False)], (0, 1))
        assert top.fetch() == [other.fetch()[0]]
        top.free()
        again = _agg(eng, both, names, "YIELD SUM($-.n), MAX($-.m)")
        assert again.fetch() == [[row[3] + other.fetch()[0][3], row[4]]]
        again.free()
        both.free()
    finally:
        a.free()
        b.free()
        other.free()


def test_profile_reports_the_kernels(vt):
    eng = vt.ld.eng
    eng.profile(True)
    _agg(eng, vt.rows, vt.names, "YIELD SUM($-.i), COUNT(*) WHERE $-.g > 0").free()
    prof = eng.profile_read()
    eng.profile(False)
    assert prof["k_ya_reduce"]["launches"] == 1 and prof["k_ya_finish"]["launches"] == 1
    assert prof["k_ya_reduce"]["ms"] > 0 and prof["k_ya_reduce"]["algo_bytes"] >= vt.t.n * 8 * 2
    assert all(prof[k]["launches"] == 0 for k in prof if k.startswith(("k_yr_", "k_so_", "k_ob_")))


# ------------------------------------------------------------------------------ scale
PER_SRC = 512
BIG_ROWS = 4_600_000 // PER_SRC * PER_SRC


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(47)
    n = BIG_ROWS
    f = Fixture()
    f.t = rt.Table([("i", rt.INT, rng.integers(rt.INT64_MIN, rt.INT64_MAX, n, endpoint=True)),
                    ("g", rt.INT, rng.integers(0, 1000, n)),
                    ("x", rt.DOUBLE, (rng.integers(-(1 << 50), 1 << 50, n) / 1024.0).view(np.uint64))], per_src=PER_SRC)
    f.ld = rt.load_numeric_table(f.t)
    yield f
    f.ld.close()


def test_scale(big):
    """About 4.6 M rows: more chunks than workgroups, a ragged last chunk, a WHERE keeping about half."""
    eng, t = big.ld.eng, big.t
    raw = eng.go_device([rt.SRC0 + s for s in range(BIG_ROWS // PER_SRC)], [rt.E_TYPE], 1, b"", big.ld.yields)
    one = None
    text = ("YIELD COUNT(*), SUM($-.i * 3 + $-.g), MAX($-.i), MIN($-.x), BIT_XOR($-.i), SUM($-.x), AVG($-.x), "
            "COUNT_DISTINCT($-.g) WHERE $-.g < 500 && $-.pos % 97 != 0")
    try:
        segs = big.ld.segments(raw)
        assert sum(-(-m // OB_CHUNK) for _, m in segs) > STAGE_GRID, "more chunks than workgroups: the grid stride runs"
        assert any(m % OB_CHUNK and m % BLOCK for _, m in segs), "a ragged last chunk"
        n_one = BIG_ROWS - 777
        one = eng.order_by(raw, big.ld.names, [("pos", False)], (0, n_one))
        for rows, n in ((raw, BIG_ROWS), (one, n_one)):
            pos = np.arange(n)
            keep = np.nonzero((t.bits["g"][pos] < 500) & (pos % 97 != 0))[0]
            assert 0.4 * n < len(keep) < 0.6 * n
            i, g, x = t.bits["i"][keep], t.bits["g"][keep], t.bits["x"][keep]
            with np.errstate(over="ignore"):
                exps = [_expect("COUNT", i, rt.INT), _expect("SUM", i * 3 + g, rt.INT), _expect("MAX", i, rt.INT),
                        _expect("MIN", x, rt.DOUBLE), _expect("BIT_XOR", i, rt.INT), _expect("SUM", x, rt.DOUBLE),
                        _expect("AVG", x, rt.DOUBLE), Exp(L.V_INT, len(np.unique(g)))]
            got, kinds = _one_row(eng, _agg(eng, rows, big.ld.names, text))
            for k, (gb, kd, e) in enumerate(zip(got, kinds, exps)):
                _check(gb, kd, e, f"scale column {k} [{'raw' if rows is raw else 'one'}]")
    finally:
        raw.free()
        if one is not None:
            one.free()
