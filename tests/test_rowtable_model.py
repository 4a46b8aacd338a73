"""Pins the numpy reference of tests/support/rowtable.py (order_ref, window_ref, group_ref: the
checkers of the value-domain and scale GPU tests) to the plain-Python models orderby.order_model
and groupby.group_model, which tests/test_orderby_model.py and tests/test_groupby_model.py pin to
the reference's own golden vectors.  The table is rowtable.value_table without NaN cells (Python's
max() and sort break on NaN; how NaNs order and group is include/nbg.h's own rule, not the
reference's); the models' rows go through the same comparison the GPU tests apply to the device's
rows (check_order, check_groups).  The value table's records are also loaded into the CPU oracle,
whose GO must yield the table bit for bit — NaN payloads included.  CPU only."""
import numpy as np
import pytest

from tests.support import groupby, orderby, rowtable as rt
from tests.support.ngql import Interim


@pytest.fixture(scope="module")
def vt():
    t = rt.value_table(nan=False)
    inp, types = t.interim()
    return t, inp, types


def test_value_table_shape():
    t = rt.value_table()
    i, x = t.bits["i"], t.bits["x"].view(np.uint64)
    for v in rt.INT_SPECIALS + rt.ladder_cells(False) + rt.ladder_cells(True):
        assert (i == v).sum() >= 2, v                      # ties exist, a LIMIT can cut them
    for v in rt.DOUBLE_SPECIALS + rt.NANS:
        assert (x == np.uint64(v)).sum() >= 2, hex(v)
    assert set(t.strings) == set(rt.STRS) and set(t.bits["d"].tolist()) == set(rt.VIDS)
    assert set(t.bits["z"].view(np.uint64).tolist()) == {0, 1 << 63}
    # the ladder: family j's images agree above byte j and differ first at byte j, bins 0x00 and 0xFF
    for j in range(7):
        imgs = rt.ladder_images(j)
        assert len({m >> (8 * (j + 1)) for m in imgs}) == 1
        assert {(m >> (8 * j)) & 255 for m in imgs} >= {0x00, 0xFF} and len({m & ((1 << (8 * j)) - 1) for m in imgs}) == 1
    # both ladder blocks lie inside the lowest / highest eighth of the order: a selection reaches them
    k = np.sort(rt.order_key(i, rt.INT))
    top = max(rt.order_key(np.array(rt.ladder_cells(False), np.int64), rt.INT).tolist())
    assert (k <= np.uint64(top)).sum() * 8 <= t.n
    # the total-order image of the NaNs: negative ones below -inf, positive ones above +inf
    xk = rt.order_key(np.array(rt.NANS + [rt.dbits(float("-inf")), rt.dbits(float("inf"))], np.uint64).view(np.int64), rt.DOUBLE)
    assert [int(a) for a in np.argsort(xk)] == [4, 1, 5, 6, 3, 0, 2]
    assert rt.NANS[4] == rt.LOWEST_NAN and rt.NANS[2] == rt.HIGHEST_NAN


def test_oracle_rows_are_the_table():
    t = rt.value_table()
    kb, schema = rt.value_records(t)
    ld = rt.load_oracle(t, kb, schema)          # asserts the oracle's GO rows == the table, by bits
    some = t.rows_of_sources(3, 5)
    rt._check_is_table(t, rt.oracle_bits(ld, t.source_vids(some)), some)
    ld.close()


ORDER_SHAPES = [
    [("i", False)], [("i", True)], [("x", False)], [("x", True)], [("d", False)], [("d", True)], [("s", False)],
    [("s", True)], [("t", False)], [("b", True)], [("z", False)], [("c", False)],
    [("z", False), ("i", True)], [("b", False), ("x", False)], [("s", True), ("d", False)],
]


@pytest.mark.parametrize("factors", ORDER_SHAPES, ids=lambda f: "_".join(n + ("-" if d else "") for n, d in f))
def test_order_ref_is_the_model(vt, factors):
    t, inp, _ = vt
    mod = orderby.order_model(inp, factors).rows
    cols, _ = rt.rows_to_bits(t, mod, len(t.names))
    rt.check_order(dict(zip(t.names, cols)), t, factors)
    for off, cnt in ((0, 7), (100, 333), (t.n - 3, 10), (5, (1 << 63) - 1), ((1 << 63) - 1, 1), (t.n, 1), (3, 0)):
        win = orderby.limit_model(Interim(inp.columns, mod), off, cnt).rows
        assert rt.window_ref(t.n, off, cnt) == orderby.window(t.n, off, cnt)
        if win:
            cols, _ = rt.rows_to_bits(t, win, len(t.names))
            rt.check_order(dict(zip(t.names, cols)), t, factors, (off, cnt))
        else:
            assert rt.window_ref(t.n, off, cnt) == (0, 0)


def test_order_ref_exact_with_every_column(vt):
    t, inp, _ = vt
    factors = [(c, k % 2 == 1) for k, c in enumerate(t.names) if c != "pos"] + [("pos", False)]
    mod = orderby.order_model(inp, factors).rows
    cols, _ = rt.rows_to_bits(t, mod, len(t.names))
    rt.check_order(dict(zip(t.names, cols)), t, factors, exact=True)


def test_check_order_rejects_wrong_rows(vt):
    t, inp, _ = vt
    f = [("b", False)]
    good = {c: t.bits[c][rt.order_ref(t, f)] for c in t.names}
    rt.check_order(good, t, f)
    bad = {c: v.copy() for c, v in good.items()}
    bad["i"][5] ^= 1                                       # a cell that is not the input row's
    with pytest.raises(AssertionError):
        rt.check_order(bad, t, f)
    dup = {c: v.copy() for c, v in good.items()}
    for c in t.names:
        dup[c][1] = dup[c][0]                              # a row twice
    with pytest.raises(AssertionError):
        rt.check_order(dup, t, f)
    rev = {c: v[::-1].copy() for c, v in good.items()}     # the keys out of order
    with pytest.raises(AssertionError):
        rt.check_order(rev, t, f)


AGGS = [("COUNT", None), ("SUM", "i"), ("AVG", "i"), ("MAX", "i"), ("MIN", "i"), ("BIT_AND", "i"), ("BIT_OR", "i"),
        ("BIT_XOR", "i"), ("STD", "i"), ("SUM", "d"), ("SUM", "t"), ("MAX", "d"), ("MIN", "t"), ("MAX", "x"), ("MIN", "x"),
        ("MAX", "s"), ("MIN", "s"), ("MAX", "b"), ("COUNT_DISTINCT", "x"), ("COUNT_DISTINCT", "i"), ("COUNT_DISTINCT", "s"),
        ("COUNT_DISTINCT", "z"), ("SUM", "s"), ("AVG", "b"), ("STD", "d"), ("BIT_OR", "x"), ("SUM", "z")]
GROUP_KEYS = [[], ["i"], ["x"], ["d"], ["s"], ["t"], ["b"], ["z"], ["c"], ["g"], ["x", "i"], ["s", "d"]]


def _sentence(keys, aggs):
    ys = [f"$-.{k} AS k_{k}" for k in keys] + [f"{f}({'*' if c is None else '$-.' + c})" for f, c in aggs]
    return groupby.parse_sentence(f"GROUP BY {', '.join('$-.' + k for k in keys) or 'abs(5)'} YIELD {', '.join(ys)}")


@pytest.mark.parametrize("keys", GROUP_KEYS, ids=lambda k: "_".join(k) or "const")
def test_group_ref_is_the_model(vt, keys):
    t, inp, types = vt
    sent = _sentence(keys, AGGS)
    mod = groupby.group_model(inp, sent.groups, sent.yields, types).rows
    cols, kinds = rt.rows_to_bits(t, mod, len(keys) + len(AGGS))
    rt.check_groups(cols, kinds, t, keys, rt.group_ref(t, keys, AGGS), what=str(keys))


def test_group_ref_double_sums(vt):
    """SUM / AVG / STD of doubles by the label column: the model adds in row order, group_ref is
    the exactly rounded sum; they agree within the bound the GPU tests use, and by class where a
    group holds infinities."""
    t, inp, types = vt
    aggs = [("COUNT", None), ("SUM", "x"), ("AVG", "x")]
    sent = _sentence(["g"], aggs)
    ref = rt.group_ref(t, ["g"], aggs)
    by_g = dict(zip(ref.keys[0].tolist(), ref.cols[1].bits.view(np.float64).tolist()))
    assert by_g[201] == float("inf") and by_g[204] == float("-inf") and np.isnan(by_g[202])
    assert by_g[205] == 1e-323 and by_g[206] == 0.0 and rt.dbits(by_g[207]) == 1 << 63
    mod = groupby.group_model(inp, sent.groups, sent.yields, types).rows
    cols, kinds = rt.rows_to_bits(t, mod, 1 + len(aggs))
    rt.check_groups(cols, kinds, t, ["g"], ref)
    # STD of doubles where the premise of the n * 2^-52 rule holds: exact sums, so one mean
    some = np.nonzero(t.bits["g"] == rt.G_EXACT)[0]
    sub = Interim(inp.columns, [inp.rows[r] for r in some])
    sent = _sentence(["g"], [("STD", "x"), ("STD", "i")])
    mod = groupby.group_model(sub, sent.groups, sent.yields, types).rows
    cols, kinds = rt.rows_to_bits(t, mod, 3)
    rt.check_groups(cols, kinds, t, ["g"], rt.group_ref(t, ["g"], [("STD", "x"), ("STD", "i")], rows=some))


def test_check_groups_rejects_wrong_values(vt):
    t, _, _ = vt
    aggs = [("COUNT", None), ("SUM", "i"), ("SUM", "x")]
    ref = rt.group_ref(t, ["g"], aggs)
    good = [ref.keys[0].copy()] + [c.bits.copy() for c in ref.cols]
    kinds = [0, 0, 0, 1]
    rt.check_groups(good, kinds, t, ["g"], ref)
    for col, delta in ((1, 1), (2, 1), (0, 1)):
        bad = [c.copy() for c in good]
        bad[col][3] += delta
        with pytest.raises(AssertionError):
            rt.check_groups(bad, kinds, t, ["g"], ref)
    at = int(np.nonzero(ref.keys[0] == rt.G_FINITE)[0][0])
    bad = [c.copy() for c in good]
    w = bad[3].view(np.float64)
    w[at] += 4 * ref.cols[2].tol[at] + abs(w[at]) * 2.0 ** -40       # outside the summation bound
    with pytest.raises(AssertionError):
        rt.check_groups(bad, kinds, t, ["g"], ref)
    with pytest.raises(AssertionError):
        rt.check_groups([c[:-1] for c in good], kinds, t, ["g"], ref)
