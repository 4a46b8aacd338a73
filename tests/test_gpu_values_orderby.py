"""nbg_order_by over the value domain: the cells tests/test_gpu_orderby.py's RMAT rows never hold.

The input is rowtable.value_table on the device (tests/support/rowtable.py): INT64_MIN / INT64_MAX
and their neighbours, a byte ladder (families of ints that agree in every byte above byte j and
differ first at byte j, with members in bins 0x00 and 0xFF of that byte, for every j), doubles as
bit patterns (zeros, subnormals, DBL_MIN, DBL_MAX, infinities of both signs and five NaNs),
negative and extreme VIDs, a TIMESTAMP and a BOOL column, and strings that are empty, prefixes of
each other and hold bytes >= 0x80.  The GO's rows are asserted to be the table bit for bit, and the
CPU oracle's too.  Expected orders come from rowtable.order_ref (numpy, written from include/nbg.h;
pinned on the CPU by tests/test_rowtable_model.py), never from the device; results are compared
by bits (DeviceRows.fetch_bits) with rowtable.check_order, which is orderby.check_window over bit
columns.  NaN factors are unspecified in the reference; nbg.h orders them by their bits' IEEE
total-order image, and that is what is held here.

The first-K selection runs when K * OB_SELECT_RATIO <= rows, so only the lowest eighth of an order
is within its reach: the ladder has a block at the low end of the int order and its mirror image
at the high end, which DESC (the complemented image) brings to the front."""
import numpy as np
import pytest

from tests.support import rowtable as rt

pytestmark = pytest.mark.gpu

SELECT_RATIO = 8       # csrc/nbg_internal.h OB_SELECT_RATIO
INT64_MAX = rt.INT64_MAX


class Fixture:
    pass


@pytest.fixture(scope="module")
def vo():
    f = Fixture()
    f.t = rt.value_table()
    f.ld = rt.load_value_table(f.t)                 # asserts the oracle's rows are the table
    f.rows, f.cols = rt.go_checked(f.ld)            # asserts the device's rows are the table
    assert len(f.ld.segments(f.rows)) >= 2          # the GO's own multi-segment result
    f.digest = f.rows.digest()
    yield f
    assert f.rows.digest() == f.digest              # the input stayed unchanged
    f.rows.free()
    f.ld.close()


COLUMNS = ["pos", "i", "x", "d", "s", "t", "b", "z", "c", "g"]


# ------------------------------------------------------------------------------ 1. one factor
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("col", COLUMNS)
def test_single_factor(vo, col, desc):
    assert vo.t.names == COLUMNS
    f = [(col, desc)]
    rt.check_order(vo.ld.order(vo.rows, f), vo.t, f)


# ------------------------------------------------------------------------------ 2. every column
def test_all_columns_exact(vo):
    """Every column a factor (pos last): the order is fixed, row for row."""
    f = [(c, k % 2 == 1) for k, c in enumerate(COLUMNS) if c != "pos"] + [("pos", True)]
    rt.check_order(vo.ld.order(vo.rows, f), vo.t, f, exact=True)


# ------------------------------------------------------------------------------ 3. a tied first factor
MULTI = {
    "zeros_ladder_desc": [("z", False), ("i", True)],      # both zeros and nothing else: they must not decide
    "bool_double": [("b", False), ("x", False)],           # two keys, then NaNs and infinities decide
    "string_desc_vid": [("s", True), ("d", False)],        # two vids share a string
    "const_double_desc_pos": [("c", True), ("x", True), ("pos", False)],
}


@pytest.mark.parametrize("shape", list(MULTI))
def test_multi_factor(vo, shape):
    f = MULTI[shape]
    rt.check_order(vo.ld.order(vo.rows, f), vo.t, f, exact=f[-1][0] == "pos")


# ------------------------------------------------------------------------------ 4. the selection
def _select(vo, factors, limit):
    """ORDER BY | LIMIT that must take the first-K selection (nbg_profile_read tells), checked."""
    lo, hi = rt.window_ref(vo.t.n, *limit)
    assert hi > lo and hi * SELECT_RATIO <= vo.t.n, "the window is outside the selection's reach"
    vo.ld.eng.profile(True)
    dev = vo.ld.order(vo.rows, factors, limit)
    prof = vo.ld.eng.profile_read()
    vo.ld.eng.profile(False)
    assert prof["k_ob_hist"]["launches"] == 8 and prof["k_ob_pick"]["launches"] == 8
    assert prof["k_ob_compact"]["launches"] == 1 and prof["k_ob_iota"]["launches"] == 0
    rt.check_order(dev, vo.t, factors, limit)
    return dev


def _run_of(vo, col, desc, cell_bits):
    """[a, b): where the rows holding `cell_bits` in `col` stand in ORDER BY col [DESC]."""
    keys = np.sort(rt.order_key(vo.t.bits[col], vo.t.types[col], desc))
    k = rt.order_key(np.array([cell_bits], np.uint64).view(np.int64), vo.t.types[col], desc)[0]
    a, b = int(np.searchsorted(keys, k, "left")), int(np.searchsorted(keys, k, "right"))
    assert b - a >= 2
    return a, b, k, keys


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("digit", [0x00, 0xFF], ids=["bin00", "binFF"])
@pytest.mark.parametrize("j", range(8))
def test_selection_decided_at_byte(vo, j, digit, desc):
    """The K-th image belongs to ladder family j: k_ob_hist / k_ob_pick tell it from its siblings
    at the pass over byte j and not before.  Asserted from the table's own keys: the rows whose key
    agrees with the K-th above byte j hold several digits at byte j, and those that agree down to
    byte j are the K-th key's tie run."""
    imgs = rt.ladder_images(j)
    img = imgs[0] if digit == 0x00 else imgs[-1]        # (family 7: its lowest and highest top byte)
    if desc:
        img = ~img & ((1 << 64) - 1)                    # the mirrored block, first under DESC
    cell = img ^ (1 << 63)
    a, b, k, keys = _run_of(vo, "i", desc, cell)
    above = np.uint64(0) if j == 7 else ~np.uint64(0) << np.uint64(8 * (j + 1))
    same_above = keys[(keys ^ k) & above == 0]
    assert len(np.unique((same_above >> np.uint64(8 * j)) & np.uint64(255))) > 1
    down_to_j = keys[(keys ^ k) & (~np.uint64(0) << np.uint64(8 * j)) == 0]
    assert (down_to_j == k).all() and len(down_to_j) == b - a
    _select(vo, [("i", desc)], (max(0, a - 2), a + 2 - max(0, a - 2)))       # K cuts the tie run


def test_selection_k_on_a_tie_runs_edges(vo):
    a, b, _, _ = _run_of(vo, "i", False, (rt.INT64_MIN + 1) & ((1 << 64) - 1))
    assert a > 0
    _select(vo, [("i", False)], (0, a + 1))            # K is the run's first row
    _select(vo, [("i", False)], (0, b))                # K is its last
    _select(vo, [("i", False)], (a, b - a))            # exactly the run
    _select(vo, [("i", False), ("x", True)], (1, b))   # the next factor orders inside the runs


KTH = {
    "int64_min": ("i", False, rt.INT64_MIN & ((1 << 64) - 1)),
    "int64_max": ("i", True, rt.INT64_MAX),
    "neg_inf": ("x", False, rt.dbits(float("-inf"))),
    "pos_inf": ("x", True, rt.dbits(float("inf"))),
    "lowest_nan": ("x", False, rt.LOWEST_NAN),
    "highest_nan": ("x", True, rt.HIGHEST_NAN),
    "vid_min": ("d", False, rt.INT64_MIN & ((1 << 64) - 1)),
    "vid_max": ("d", True, rt.INT64_MAX),
    "empty_string": ("s", False, 0),
}


@pytest.mark.parametrize("case", list(KTH))
def test_selection_kth_key_is_an_extreme(vo, case):
    col, desc, cell = KTH[case]
    a, b, k, keys = _run_of(vo, col, desc, cell)
    if case in ("int64_min", "int64_max", "lowest_nan", "highest_nan", "vid_min", "vid_max", "empty_string"):
        assert a == 0                                   # nothing sorts before it
    if case in ("neg_inf", "pos_inf"):
        x = vo.t.bits["x"].view(np.float64)             # only the NaNs of that sign do
        assert a == (np.isnan(x) & (np.signbit(x) == (case == "neg_inf"))).sum() >= 6
    dev = _select(vo, [(col, desc)], (0, a + 2))
    assert rt.order_key(dev[col], vo.t.types[col], desc)[-1] == k
    _select(vo, [(col, desc), ("pos", True)], (a + 1, 1))


def test_selection_constant_first_factor(vo):
    """Every row is a candidate: the selection keeps them all and the later factors order them."""
    _select(vo, [("c", False), ("i", False)], (0, 50))
    _select(vo, [("z", True), ("x", False), ("pos", False)], (17, 100))     # zeros of both signs: one key


# ------------------------------------------------------------------------------ 5. saturating LIMIT
@pytest.mark.parametrize("shape", ["i", "x_desc", "s_d", "limit_only"])
def test_limit_saturates(vo, shape):
    f = {"i": [("i", False)], "x_desc": [("x", True)], "s_d": [("s", False), ("d", True)], "limit_only": []}[shape]
    n = vo.t.n
    for off, cnt in ((5, INT64_MAX), (INT64_MAX, 1), (INT64_MAX, INT64_MAX), (n - 1, INT64_MAX), (n, INT64_MAX), (0, INT64_MAX)):
        dev = vo.ld.order(vo.rows, f, (off, cnt))
        assert len(dev["pos"]) == max(0, n - off)
        if f:
            rt.check_order(dev, vo.t, f, (off, cnt))
        else:                                           # LIMIT only: the input's own fetch order
            for c in COLUMNS:
                assert np.array_equal(dev[c], vo.cols[c][off:])
