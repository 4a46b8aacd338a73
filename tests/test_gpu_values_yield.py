"""nbg_yield over chosen cells, at the row counts where its kernels take another path, and at
scale.  Inputs are rowtable tables (tests/support/rowtable.py): a one-step GO from chosen sources
yields exactly the table's rows, `pos` identifies a row, and `order_by(pos)` is the same input as
one segment.  Expected rows come from the plain-Python model of tests/support/yieldpipe.py over
the table's own cells — or, at scale, from numpy over them — never from the device.

The value table is that of tests/test_gpu_values_setops.py: i (INT: the int64 extremes, 2^53 + 1),
d (VID, both signs and the extremes), s (STRING, bytes >= 0x80 among them), t (TIMESTAMP), x
(DOUBLE: every special of both signs, both zeros, NaNs of both signs and several payloads), xs
(DOUBLE cells whose cast to an integer is defined) and b (BOOL).

Doubles are compared by their bits.  One class of cells is compared as "a NaN" only: a NaN that an
arithmetic instruction produced (x + 1.0, x * 2, x / 3, x % 2 over a NaN or an invalid operation).
IEEE 754 leaves the payload and sign of such a result to the implementation, and the model's
arithmetic runs on the host's FPU.  A NaN that is passed through, or negated (a sign-bit flip),
keeps its bits and is compared by them."""
import math

import numpy as np
import pytest

from nebula_amd import NbgError, _lib as L, expr as E
from tests.support import ngql, rowtable as rt, setops, yieldpipe
from tests.support.groupby import AggCol
from tests.test_gpu_values_setops import COUNTS, _value_table

pytestmark = pytest.mark.gpu

BLOCK = 256                    # csrc/ws.h
OB_CHUNK, STAGE_GRID = 2048, 2048   # csrc/nbg_internal.h, csrc/stage.h


class Fixture:
    pass


def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


def P(name):
    return E.input_prop(name)


def K(v):
    return E.const(v)


def B(op, a, b):
    return E.binop(op, a, b)


def _sentence(cols, where=None):
    """cols: [(alias, expr)]."""
    return yieldpipe.YieldSentence([AggCol("", e, a) for a, e in cols], where)


def _run(eng, rows, names, st):
    return eng.yield_rows(rows, names, [c.expr.encode() for c in st.yields], st.where.encode() if st.where is not None else b"")


def _cells(rows, loose=()):
    """Rows as comparable cells: the kind and the value, doubles by their bits; the columns in `loose`
    hold arithmetic results, whose NaNs compare as NaNs (see the module text)."""
    out = []
    for r in rows:
        row = []
        for c, v in enumerate(r):
            if isinstance(v, float) and math.isnan(v) and c in loose:
                row.append(("double", "nan"))
            else:
                row.append(setops.bits_cell(v))
        out.append(tuple(row))
    return out


# ------------------------------------------------------------------------------ the value table
@pytest.fixture(scope="module")
def vt():
    f = Fixture()
    f.t = _value_table()
    f.ld = rt.load_value_table(f.t)
    f.rows, _ = rt.go_checked(f.ld)           # the GO's rows are the table's, bit for bit
    f.names = f.ld.names
    f.inp = ngql.Interim(f.names, f.rows.fetch())
    f.one = f.ld.by_pos(f.rows)               # the same rows as one segment, in table order
    f.inp_one = ngql.Interim(f.names, f.one.fetch())
    assert [r[0] for r in f.inp_one.rows] == list(range(f.t.n)) and f.t.n == sum(COUNTS)
    yield f
    f.rows.free()
    f.one.free()
    f.ld.close()


WHERE = B("!=", B("%", P("pos"), K(3)), K(1))
# per column: ([(alias, expr)], the result columns that hold arithmetic doubles)
VALUE_COLUMNS = {
    "i": ([("pos", P("pos")), ("a", B("+", P("i"), K(1))), ("m", B("*", P("i"), K(3))), ("n", E.unary("-", P("i"))),
           ("s", B("-", P("i"), P("pos"))), ("q", B("/", P("i"), K(7))), ("r", B("%", P("i"), K(-7))),
           ("x", B("^", P("i"), P("pos"))), ("f", E.cast("double", P("i"))), ("b", E.cast("bool", P("i"))),
           ("lt", B("<", P("i"), K(0))), ("eq", B("==", P("i"), P("d"))), ("ge", B(">=", P("i"), P("t"))),
           ("fd", B("/", P("i"), K(2.0))), ("fe", B("==", P("i"), K(9007199254740992.0)))], ()),
    "d": ([("pos", P("pos")), ("d", P("d")), ("m", B("%", P("d"), K(5))), ("h", E.Expr(E.K_FUNC, alias="hash", args=[P("d")])),
           ("gt", B(">", P("d"), P("i"))), ("n", E.unary("-", P("d")))], ()),
    "s": ([("pos", P("pos")), ("s", P("s")), ("eq", B("==", P("s"), K("ab"))), ("lt", B("<", P("s"), K("abc"))),
           ("ge", B(">=", P("s"), K("é"))), ("ne", B("!=", P("s"), K(""))), ("le", B("<=", P("s"), K("\x7f"))),
           ("gx", B(">", P("s"), K("not in the dictionary")))], ()),
    "t": ([("pos", P("pos")), ("t", P("t")), ("a", B("+", P("t"), K(1))), ("f", E.cast("double", P("t"))),
           ("z", B("==", P("t"), K(0))), ("c", E.cast("timestamp", B("*", P("t"), K(2))))], ()),
    "x": ([("pos", P("pos")), ("x", P("x")), ("n", E.unary("-", P("x"))), ("a", B("+", P("x"), K(1.0))),
           ("m", B("*", P("x"), K(2))), ("q", B("/", P("x"), K(3))), ("r", B("%", P("x"), K(2))),
           ("lt", B("<", P("x"), K(0))), ("le", B("<=", P("x"), K(1))), ("gt", B(">", P("x"), K(0.0))),
           ("ge", B(">=", P("x"), P("xs"))), ("eq", B("==", P("x"), P("x"))), ("ne", B("!=", P("x"), K(1.0))),
           ("b", E.cast("bool", P("x"))), ("nb", E.unary("!", P("x"))), ("dz", B("/", K(1.0), P("x")))], (3, 4, 5, 6, 15)),
    "xs": ([("pos", P("pos")), ("c", E.cast("int", P("xs"))), ("b", E.cast("bool", P("xs"))), ("t", E.cast("timestamp", P("xs"))),
            ("d", E.cast("double", P("xs"))), ("p", B("+", E.cast("int", P("xs")), P("pos")))], ()),
    "b": ([("pos", P("pos")), ("n", E.unary("!", P("b"))), ("c", E.cast("int", P("b"))), ("f", E.cast("double", P("b"))),
           ("a", B("&&", P("b"), B(">", P("i"), K(0)))), ("o", B("||", P("b"), B("<", P("x"), K(0)))),
           ("x", B("XOR", P("b"), P("i"))), ("e", B("==", P("b"), K(1))), ("l", B("<", P("b"), K(True)))], ()),
}


@pytest.mark.parametrize("col", list(VALUE_COLUMNS))
def test_value_cells(vt, col):
    """Arithmetic, comparisons and casts over every cell of one column: the ragged raw GO result and
    the same rows as one segment, cell by cell against the model."""
    cols, loose = VALUE_COLUMNS[col]
    st = _sentence(cols, WHERE)
    for rows, inp in ((vt.rows, vt.inp), (vt.one, vt.inp_one)):
        want, _ = yieldpipe.yield_model(inp, st)
        out = _run(vt.ld.eng, rows, vt.names, st)
        dev = out.fetch()
        out.free()
        assert len(dev) == len(want.rows) == sum(1 for r in inp.rows if r[0] % 3 != 1)
        assert [r[0] for r in dev] == [r[0] for r in want.rows]            # rows identified by pos, in the input's order
        assert _cells(dev, loose) == _cells(want.rows, loose)


def test_value_table_shows_what_it_should(vt):
    x = vt.inp.columns.index("x")
    nans = {rt.dbits(r[x]) for r in vt.inp.rows if math.isnan(r[x])}
    assert nans == set(rt.NANS) and any(rt.dbits(r[x]) == 1 << 63 for r in vt.inp.rows)
    i = vt.inp.columns.index("i")
    assert {rt.INT64_MIN, rt.INT64_MAX, (1 << 53) + 1} <= {r[i] for r in vt.inp.rows}
    s = vt.inp.columns.index("s")
    assert any(any(ch >= 0x80 for ch in r[s].encode()) for r in vt.inp.rows) and any(r[s] == "" for r in vt.inp.rows)
    assert vt.ld.eng.lib.nbg_rows_num_segments(vt.rows.h) >= 2


def test_passed_through_columns_keep_every_bit(vt):
    st = _sentence([("all", E.input_prop("*"))])
    for rows, inp in ((vt.rows, vt.inp), (vt.one, vt.inp_one)):
        out = _run(vt.ld.eng, rows, vt.names, st)
        assert vt.ld.kinds_of(out) == vt.ld.kinds_of(rows)
        dev = out.fetch()
        out.free()
        assert _cells(dev) == _cells(inp.rows)


def test_one_failing_row(vt):
    """`$-.i / ($-.pos - K)` fails on exactly one row, pos == K."""
    i = vt.inp_one.columns.index("i")
    k = next(k for k in range(500, vt.t.n) if vt.inp_one.rows[k - 1][i] != rt.INT64_MIN)     # (INT64_MIN / -1 fails too)
    div = B("/", P("i"), B("-", P("pos"), K(k)))
    failing = [r[0] for r in vt.inp_one.rows if r[0] == k or (r[i] == rt.INT64_MIN and r[0] - k == -1)]
    assert failing == [k]
    eng = vt.ld.eng
    for rows, inp in ((vt.rows, vt.inp), (vt.one, vt.inp_one)):
        # in the WHERE
        assert _code(lambda: _run(eng, rows, vt.names, _sentence([("pos", P("pos"))], B(">=", div, K(0))))) == L.E_EXECUTION_ERROR
        # in a YIELD of a passing row
        assert _code(lambda: _run(eng, rows, vt.names, _sentence([("pos", P("pos")), ("q", div)]))) == L.E_EXECUTION_ERROR
        assert _code(lambda: _run(eng, rows, vt.names, _sentence([("q", div)], B("<=", P("pos"), K(k))))) == L.E_EXECUTION_ERROR
        # in a YIELD of a rejected row: no error
        st = _sentence([("pos", P("pos")), ("q", div)], B("!=", P("pos"), K(k)))
        out = _run(eng, rows, vt.names, st)
        dev = out.fetch()
        out.free()
        assert len(dev) == vt.t.n - 1 and _cells(dev) == _cells(yieldpipe.yield_model(inp, st)[0].rows)


def test_32_columns(vt):
    names = ("i", "x", "b", "t", "xs", "d", "s", "pos")
    cols = [(f"c{k}", P(names[k % 8]) if k % 3 else B("+", P("pos"), K(k))) for k in range(32)]
    st = _sentence(cols, B("!=", B("%", P("pos"), K(5)), K(0)))
    want, _ = yieldpipe.yield_model(vt.inp, st)
    out = _run(vt.ld.eng, vt.rows, vt.names, st)
    assert vt.ld.eng.lib.nbg_rows_num_cols(out.h) == 32
    dev = out.fetch()
    out.free()
    assert _cells(dev) == _cells(want.rows) and dev
    with pytest.raises(NbgError) as ex:
        _run(vt.ld.eng, vt.rows, vt.names, _sentence(cols + [("c32", P("i"))]))
    assert ex.value.code == L.E_UNSUPPORTED


def _deep(levels):
    """A right-leaning tree: one more live register per level, two instructions per level."""
    e = P("pos")
    for k in range(levels):
        e = B("-", P("i"), e) if k % 2 else B("+", P("pos"), e)
    return e


def test_register_limit(vt):
    """The deepest program the device's register file holds runs and is right; one level more is
    NBG_E_UNSUPPORTED for the register file (not for the program length).  The limit comes from the
    device's LDS (interp_max_regs, at most the compiler's 48), so it is found, not assumed."""
    eng = vt.ld.eng
    limit, msg = None, ""
    for levels in range(8, 62):
        try:
            _run(eng, vt.one, vt.names, _sentence([("pos", P("pos")), ("v", _deep(levels))], WHERE)).free()
        except NbgError as ex:
            assert ex.code == L.E_UNSUPPORTED
            limit, msg = levels, str(ex)
            break
    assert limit is not None and "register" in msg and "program too long" not in msg
    assert 14 <= limit <= 48                      # at least the 16 registers every device has held
    st = _sentence([("pos", P("pos")), ("v", _deep(limit - 1))], WHERE)
    for rows, inp in ((vt.rows, vt.inp), (vt.one, vt.inp_one)):
        out = _run(eng, rows, vt.names, st)
        dev = out.fetch()
        out.free()
        assert _cells(dev) == _cells(yieldpipe.yield_model(inp, st)[0].rows)
    # the limit holds for the WHERE part too
    assert _code(lambda: _run(eng, vt.one, vt.names, _sentence([("pos", P("pos"))], B(">", _deep(limit + 1), K(0))))) == L.E_UNSUPPORTED


# ------------------------------------------------------------------------------ row counts
ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
SRC_SIZES = np.diff([0] + ROW_COUNTS)            # sources 0..k hold ROW_COUNTS[k] rows together


@pytest.fixture(scope="module")
def ct():
    """A numeric table whose first k + 1 sources hold ROW_COUNTS[k] rows: v (INT, random) and y
    (DOUBLE, random finite)."""
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


def _patterns(n):
    """WHEREs over pos: none kept, all kept, one row (the first / the last of a chunk), alternating."""
    last = min(n, OB_CHUNK) - 1
    return {
        "none": B("<", P("pos"), K(0)),
        "all": B(">=", P("pos"), K(0)),
        "first": B("==", P("pos"), K(0)),
        "chunk_last": B("==", P("pos"), K(last)),
        "last": B("==", P("pos"), K(n - 1)),
        "alternating": B("==", B("%", P("pos"), K(2)), K(1)),
    }


@pytest.mark.parametrize("k", range(len(ROW_COUNTS)), ids=[f"rows{c}" for c in ROW_COUNTS])
def test_row_counts(ct, k):
    n = ROW_COUNTS[k]
    eng = ct.ld.eng
    raw = ct.ld.go([rt.SRC0 + s for s in range(k + 1)])
    one = ct.ld.by_pos(raw)
    try:
        assert raw.count == n == one.count
        if n >= 2047:
            assert eng.lib.nbg_rows_num_segments(raw.h) >= 2       # a ragged input: several workgroups' regions
        for rows in (raw, one):
            pos, v, y = rows.fetch_bits()                          # the input's fetch order
            if rows is one:
                assert np.array_equal(pos, np.arange(n))
            assert np.array_equal(v, ct.t.bits["v"][pos]) and np.array_equal(y, ct.t.bits["y"][pos])
            for name, where in _patterns(n).items():
                keep = {"none": pos < 0, "all": pos >= 0, "first": pos == 0, "chunk_last": pos == min(n, OB_CHUNK) - 1,
                        "last": pos == n - 1, "alternating": pos % 2 == 1}[name]
                st = _sentence([("pos", P("pos")), ("w", B("+", B("*", P("v"), K(2)), K(1))), ("y", P("y"))], where)
                out = _run(eng, rows, ct.names, st)
                assert out.count == int(keep.sum()), (n, name)
                got = out.fetch_bits()
                out.free()
                assert np.array_equal(got[0], pos[keep]), (n, name)               # the input's fetch order, filtered
                assert np.array_equal(got[1], v[keep] * 2 + 1) and np.array_equal(got[2], y[keep]), (n, name)
            # without a WHERE: a row's slot is its logical index
            out = _run(eng, rows, ct.names, _sentence([("y", P("y")), ("pos", P("pos"))]))
            got = out.fetch_bits()
            out.free()
            assert np.array_equal(got[1], pos) and np.array_equal(got[0], y)
    finally:
        raw.free()
        one.free()


# ------------------------------------------------------------------------------ scale
PER_SRC = 512
BIG_ROWS = 4_600_000 // PER_SRC * PER_SRC


@pytest.fixture(scope="module")
def big():
    """A numeric table sized as tests/test_gpu_values_setops.py's: i (INT, full range), g (INT,
    small) and x (DOUBLE, finite)."""
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
    """About 4.6 M rows: more chunks than workgroups, a ragged last chunk, a WHERE keeping about
    half.  The count, the order and the cells against numpy, over the raw GO result and over the
    ordered input (where the result's pos ascends)."""
    eng, t = big.ld.eng, big.t
    nsrc = BIG_ROWS // PER_SRC
    raw = eng.go_device([rt.SRC0 + s for s in range(nsrc)], [rt.E_TYPE], 1, b"", big.ld.yields)
    one = None
    try:
        segs = big.ld.segments(raw)
        assert sum(-(-m // OB_CHUNK) for _, m in segs) > STAGE_GRID, "more chunks than workgroups: the grid stride runs"
        assert any(m % OB_CHUNK and m % BLOCK for _, m in segs), "a ragged last chunk"
        st = _sentence([("pos", P("pos")), ("a", B("+", B("*", P("i"), K(3)), P("g"))), ("h", B("*", P("x"), K(0.5))),
                        ("lt", B("<", P("x"), K(0.0)))],
                       B("&&", B("<", P("g"), K(500)), B("!=", B("%", P("pos"), K(97)), K(0))))
        n_one = BIG_ROWS - 777                                    # one segment whose last chunk is ragged
        one = eng.order_by(raw, big.ld.names, [("pos", False)], (0, n_one))
        for rows in (raw, one):
            pos = rows.fetch_bits()[0]
            if rows is one:
                assert np.array_equal(pos, np.arange(n_one)) and n_one % OB_CHUNK and n_one % BLOCK
            keep = (t.bits["g"][pos] < 500) & (pos % 97 != 0)
            want = pos[keep]
            assert 0.4 * len(pos) < len(want) < 0.6 * len(pos)
            out = _run(eng, rows, big.ld.names, st)
            assert out.count == len(want) and eng.lib.nbg_rows_num_segments(out.h) == 1
            got = out.fetch_bits()
            out.free()
            assert np.array_equal(got[0], want)                       # the input's order (pos ascending over `one`)
            with np.errstate(over="ignore"):
                assert np.array_equal(got[1], t.bits["i"][want] * 3 + t.bits["g"][want])
            x = t.bits["x"][want].view(np.float64)
            assert np.array_equal(got[2], (x * 0.5).view(np.int64)) and np.array_equal(got[3], (x < 0.0).astype(np.int64))
    finally:
        raw.free()
        if one is not None:
            one.free()
