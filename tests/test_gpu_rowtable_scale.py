"""nbg_order_by / nbg_group_by where the row walk and the tables can go wrong: more chunks than
workgroups, segments longer than a chunk, both sides of the LDS limit, waves with 1 / 8 / 9 / 64
groups, groups across wave, workgroup and chunk boundaries, and probe chains that wrap around the
last table slot.  Inputs are rowtable tables (tests/support/rowtable.py) with chosen cells; expected
values come from rowtable's numpy reference (pinned on the CPU by tests/test_rowtable_model.py),
never from the device.  Every structural condition is asserted from the result's own segments
(nbg_rows_num_segments / nbg_rows_segment), group counts or the mirrored hash — not assumed.

The big table.  A GO's final step runs at most EXPAND_GRID = 2048 workgroups per OVER type and each
appends to one segment, so a GO result over one edge type has at most 2048 segments.  More than
OB_GRID = 2048 chunks (stage_chunks cuts every segment into pieces of OB_CHUNK = 2048 rows) therefore
needs segments longer than a chunk: a little over 2048 * 2048 rows, whatever the GO's shape.  The
fixture loads more sources than that needs and bisects, over trial GOs' segment lists, the smallest
number of sources whose result has more than OB_GRID chunks and a segment longer than OB_CHUNK
whose length is no multiple of BLOCK.
Not covered: k_gb_keys' / k_gb_accum's grid stride (more than 8192 non-empty segments) — by the
above no GO result has that many, and the outputs of nbg_group_by / nbg_order_by have one.

Probe chains (test_probe_chain_wraps_*).  `_mix` / `_key_slot` / `_distinct_slot` mirror
gb_mix64, gb_key_hash (one INT key column) and the slot expression of k_gb_distinct (no key: group
id 0) in csrc/groupby.hip, to choose keys whose home slots are the last eight of the 1024-slot
table, so that the chain runs through slot 1023 into slot 0 and every second occurrence walks it
in gb_find.  If the kernel's hash changes, the parity assertions still hold but the case stops
being adversarial: the mirror must follow the kernel."""
import numpy as np
import pytest

from tests.support import rowtable as rt

pytestmark = pytest.mark.gpu

BLOCK = 256                    # csrc/ws.h
OB_CHUNK, OB_GRID = 2048, 2048 # csrc/nbg_internal.h, csrc/orderby.hip
SELECT_RATIO = 8               # csrc/nbg_internal.h OB_SELECT_RATIO
GB_ROUNDS = 8                  # csrc/groupby.hip
GB_LDS_BYTES = 16 * 1024       # csrc/nbg_internal.h
M64 = (1 << 64) - 1


class Fixture:
    pass


def _chunks(segs):
    return sum(-(-n // OB_CHUNK) for _, n in segs)


# ------------------------------------------------------------------------------ 1 / 2. the big table
PER_SRC = 512
BIG_ROWS = 4_600_000 // PER_SRC * PER_SRC


def _big_table():
    rng = np.random.default_rng(41)
    n = BIG_ROWS
    i = rng.integers(rt.INT64_MIN, rt.INT64_MAX, n, endpoint=True)
    x = rng.integers(0, 1 << 64, n, dtype=np.uint64)              # random bit patterns: every exponent, some NaNs
    special = np.array(rt.DOUBLE_SPECIALS + rt.NANS, np.uint64)
    at = rng.choice(n, n // 50, replace=False)
    x[at] = special[rng.integers(0, len(special), len(at))]
    xf = x.copy()                                                 # the NaN-free copy
    xf[np.isnan(xf.view(np.float64))] = rt.dbits(1.0)
    g = rng.integers(0, 100_000, n) * 92_233_720_368_547 - (1 << 62)   # > 65 536 distinct, both signs
    b = rng.integers(0, 3, n)
    return rt.Table([("i", rt.INT, i), ("x", rt.DOUBLE, x), ("xf", rt.DOUBLE, xf), ("g", rt.INT, g), ("b", rt.INT, b)],
                    per_src=PER_SRC)


@pytest.fixture(scope="module")
def big():
    f = Fixture()
    f.t = _big_table()
    f.ld = rt.load_numeric_table(f.t)
    nsrc = BIG_ROWS // PER_SRC
    srcs = f.t.source_vids()

    def shape(k):
        r = f.ld.go(srcs[:k])
        segs = f.ld.segments(r)
        r.free()
        return _chunks(segs) > OB_GRID and any(n > OB_CHUNK and n % BLOCK for _, n in segs)
    assert shape(nsrc), "no GO over this table reaches more chunks than OB_GRID"
    lo, hi = 1, nsrc                                              # the smallest such number of sources
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if shape(mid) else (mid + 1, hi)
    f.idx = f.t.rows_of_sources(0, lo)
    f.n = len(f.idx)
    f.rows, f.cols = rt.go_checked(f.ld, f.idx)                   # the device's rows are the table's
    f.segs = f.ld.segments(f.rows)
    yield f
    f.rows.free()
    f.ld.close()


def test_big_structure(big):
    assert _chunks(big.segs) > OB_GRID, "more chunks than k_ob_* workgroups: the grid stride runs"
    assert any(n > OB_CHUNK and n % BLOCK for _, n in big.segs), "a segment of several chunks, the last one ragged"
    assert len(big.segs) <= 8192                                  # (k_gb_keys' grid stride: see the module docstring)
    assert len(np.unique(big.t.bits["g"][big.idx])) > 65536 and len(np.unique(big.t.bits["b"][big.idx])) == 3
    x = big.t.bits["x"][big.idx].view(np.uint64)
    assert all((x == np.uint64(s)).any() for s in rt.DOUBLE_SPECIALS + rt.NANS)


def test_big_all_columns_exact(big):
    f = [("x", True), ("g", False), ("b", True), ("xf", False), ("i", True), ("pos", False)]
    rt.check_order(big.ld.order(big.rows, f), big.t, f, rows=big.idx, exact=True)


@pytest.mark.parametrize("window", ["first", "inside", "last_selected"])
def test_big_selection_x_desc(big, window):
    k = big.n // SELECT_RATIO
    off, cnt = {"first": (0, 1000), "inside": (k // 2 + 3, 4097), "last_selected": (k - 777, 777)}[window]
    assert (off + cnt) * SELECT_RATIO <= big.n
    f = [("x", True)]
    big.ld.eng.profile(True)
    dev = big.ld.order(big.rows, f, (off, cnt))
    prof = big.ld.eng.profile_read()
    big.ld.eng.profile(False)
    assert prof["k_ob_hist"]["launches"] == 8 and prof["k_ob_compact"]["launches"] == 1 and prof["k_ob_iota"]["launches"] == 0
    rt.check_order(dev, big.t, f, (off, cnt), rows=big.idx)


def test_big_order_g_i(big):
    f = [("g", False), ("i", False)]
    rt.check_order(big.ld.order(big.rows, f), big.t, f, rows=big.idx)


def test_big_limit_only_windows(big):
    """LIMIT without ORDER BY: the fetched input's slice, for windows that start and end inside
    chunks of a long segment, cover whole segments, and end at the last row (k_ob_copy's stride and
    its chunks' third word)."""
    at, n = next((a, n) for a, n in big.segs if n > OB_CHUNK and n % BLOCK)
    wins = [(at + 5, OB_CHUNK), (at + OB_CHUNK - 3, 7), (at + 1, n - 2), (3, big.n - 4), (big.n - 5, 100),
            (big.segs[len(big.segs) // 2][0] - 1, 3 * OB_CHUNK + 2)]
    for off, cnt in wins:
        dev = big.ld.order(big.rows, [], (off, cnt))
        for c in big.t.names:
            assert np.array_equal(dev[c], big.cols[c][off:off + cnt]), (c, off, cnt)


BIG_AGGS = [("COUNT", None), ("SUM", "i"), ("MAX", "i"), ("MIN", "i"), ("MAX", "xf"), ("MIN", "xf"), ("BIT_XOR", "i"),
            ("COUNT_DISTINCT", "b"), ("AVG", "i")]


@pytest.mark.parametrize("keys", [["g"], ["b"], []], ids=["g_global", "b_lds", "const"])
def test_big_group_by(big, keys):
    ref = rt.group_ref(big.t, keys, BIG_AGGS, big.idx)
    nacc = 9                        # COUNT, and one accumulator per aggregate after it (stages.cpp's plan)
    if keys == ["g"]:
        assert ref.n > 65536 and nacc * ref.n * 8 > GB_LDS_BYTES
    if keys == ["b"]:
        assert ref.n == 3 and nacc * ref.n * 8 <= GB_LDS_BYTES
    i = big.t.bits["i"][big.idx]
    assert abs(sum(i[:100_000].tolist())) > 1 << 63               # the SUM wraps
    cols, kinds = big.ld.group(big.rows, keys, BIG_AGGS)
    rt.check_groups(cols, kinds, big.t, keys, ref, str(keys))


# ------------------------------------------------------------------------------ 3 - 5. the small table
AGGS = [("COUNT", None), ("SUM", "v"), ("MIN", "v"), ("BIT_XOR", "v"), ("SUM", "y"), ("MAX", "v"), ("MIN", "y"), ("MAX", "y")]
# the plan of nbg_group_by (stages.cpp): slot 0 is COUNT, which COUNT(*) reads; every other
# aggregate here takes one slot of its own (SUM, MIN, BIT_XOR, SUM, MAX, MIN, MAX): nacc = 1 + 7 = 8.
NACC = 8
G_LDS = GB_LDS_BYTES // (NACC * 8)          # 256 groups: 8 * 256 * 8 == GB_LDS_BYTES, the last LDS case
WAVE_GROUPS = [1, GB_ROUNDS, GB_ROUNDS + 1, 64, 64, GB_ROUNDS + 1, GB_ROUNDS, 1]


def _mix(x):
    """gb_mix64 of csrc/groupby.hip over uint64 arrays."""
    x = np.asarray(x, np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


SEED = np.uint64(0x6E6562756C61)


def _key_slot(v, mask=1023):
    """gb_key_hash for one INT key column (c = 0), masked as k_gb_keys / gb_find mask it."""
    return _mix(SEED ^ np.asarray(v).view(np.uint64) ^ np.uint64(0)) & np.uint64(mask)


def _distinct_slot(v, mask=1023):
    """k_gb_distinct's first slot for group id 0 (no key column)."""
    return _mix(_mix(np.array([SEED ^ np.uint64(0)], np.uint64))[0] ^ np.asarray(v).view(np.uint64)) & np.uint64(mask)


def _adversarial(slot_fn, seed):
    """256 distinct full-range int64 values whose home slots all lie in [1016, 1023]."""
    rng = np.random.default_rng(seed)
    cand = np.unique(rng.integers(rt.INT64_MIN, rt.INT64_MAX, 200_000, endpoint=True))
    with np.errstate(over="ignore"):
        keep = cand[slot_fn(cand) >= 1016]
    assert len(keep) >= 256
    return rng.permutation(keep)[:256]


def _cases():
    """name -> (g, v): the blocks of the small table, in row order."""
    rng = np.random.default_rng(43)
    out = {}
    for name, G in (("lds_last", G_LDS), ("global_first", G_LDS + 1)):
        out[name] = rng.permutation(np.arange(G).repeat(10)) * 1_000_003 - 77
    w = []
    for k, ng in enumerate(WAVE_GROUPS):        # 64 rows per wave, exactly ng distinct groups, shared across waves
        w.append(rng.permutation(np.resize(np.arange(ng), 64)))
    out["waves"] = np.concatenate(w)
    s = 100 + np.arange(2 * OB_CHUNK + 300) % 7
    s[60:70], s[BLOCK - 6:BLOCK + 6], s[OB_CHUNK - 8:OB_CHUNK + 8] = 1, 2, 3
    out["straddle"] = s
    for n in (BLOCK - 1, BLOCK, BLOCK + 1):
        out[f"one_group_{n}"] = np.full(n, 5)
    with np.errstate(over="ignore"):
        out["probe_keys"] = rng.permutation(_adversarial(_key_slot, 47).repeat(2))
        out["probe_distinct"] = np.full(512, 9)
        dv = rng.permutation(_adversarial(_distinct_slot, 53).repeat(2))
    g = {k: np.asarray(a, np.int64) for k, a in out.items()}
    v = {k: rng.integers(rt.INT64_MIN, rt.INT64_MAX, len(a), endpoint=True) for k, a in g.items()}
    v["probe_distinct"] = dv
    return g, v


@pytest.fixture(scope="module")
def small():
    g, v = _cases()
    f = Fixture()
    f.case_src, src, at = {}, [], 0
    for k, (name, a) in enumerate(g.items()):
        src.append(k * 1000 + np.arange(len(a)) // 97)           # sources of its own, 97 rows each
        f.case_src[name] = k * 1000
    rng = np.random.default_rng(59)
    n = sum(len(a) for a in g.values())
    y = (rng.integers(-(1 << 30), 1 << 30, n) / 8.0).view(np.uint64)      # exact double sums in any order
    f.t = rt.Table([("g", rt.INT, np.concatenate(list(g.values()))), ("v", rt.INT, np.concatenate([v[k] for k in g])),
                    ("y", rt.DOUBLE, y)], src=np.concatenate(src))
    f.ld = rt.load_numeric_table(f.t)
    yield f
    f.ld.close()


def _case(small, name, placed=True):
    """(input rows, the table rows of the case): the GO's own result, or its ORDER BY pos copy,
    whose physical row i is the case's row i."""
    idx = small.t.rows_of_sources(small.case_src[name], small.case_src[name] + 1000)
    rows, _ = rt.go_checked(small.ld, idx)
    if not placed:
        return rows, idx
    out = small.ld.by_pos(rows)
    rows.free()
    got = small.ld.bits_of(out)
    assert np.array_equal(got["pos"], idx) and np.array_equal(got["g"], small.t.bits["g"][idx])     # row i is table row i
    return out, idx


def _check(small, rows, idx, keys, aggs=AGGS, what=""):
    ref = rt.group_ref(small.t, keys, aggs, idx)
    cols, kinds = small.ld.group(rows, keys, aggs)
    rt.check_groups(cols, kinds, small.t, keys, ref, what)
    return cols, ref


@pytest.mark.parametrize("name", ["lds_last", "global_first"])
def test_lds_boundary(small, name):
    rows, idx = _case(small, name, placed=False)
    try:
        assert len(small.ld.segments(rows)) >= 2
        cols, ref = _check(small, rows, idx, ["g"], what=name)
        if name == "lds_last":
            assert NACC * len(cols[0]) * 8 == GB_LDS_BYTES           # the last group count that takes the LDS
        else:
            assert NACC * (len(cols[0]) - 1) * 8 == GB_LDS_BYTES     # one more: the global accumulators
    finally:
        rows.free()


def test_waves_with_1_8_9_64_groups(small):
    rows, idx = _case(small, "waves")
    try:
        g = small.ld.bits_of(rows)["g"]
        assert [len(np.unique(g[w * 64:(w + 1) * 64])) for w in range(len(WAVE_GROUPS))] == WAVE_GROUPS
        assert GB_ROUNDS in WAVE_GROUPS and GB_ROUNDS + 1 in WAVE_GROUPS     # the last combined round, the first lane alone
        _check(small, rows, idx, ["g"], what="waves")
        _check(small, rows, idx, [], what="waves, no key")
    finally:
        rows.free()


def test_group_across_wave_workgroup_and_chunk_boundaries(small):
    rows, idx = _case(small, "straddle")
    try:
        g = small.ld.bits_of(rows)["g"]
        for key, edge in ((1, 64), (2, BLOCK), (3, OB_CHUNK)):
            at = np.nonzero(g == key)[0]
            assert at.min() < edge <= at.max() and len(at) == at.max() - at.min() + 1      # one run across the edge
        _check(small, rows, idx, ["g"], what="straddle")
    finally:
        rows.free()


@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_one_group_of_block_rows(small, n):
    rows, idx = _case(small, f"one_group_{n}")
    try:
        assert rows.count == n
        cols, _ = _check(small, rows, idx, ["g"], what=f"{n} rows")
        assert len(cols[0]) == 1 and cols[1][0] == n
        _check(small, rows, idx, [], what=f"{n} rows, no key")
    finally:
        rows.free()


def test_probe_chain_wraps_group_table(small):
    """256 keys, each twice, whose home slots (the mirror of gb_key_hash) are the table's last
    eight: linear probing fills 1016..1023 and wraps into 0..247."""
    rows, idx = _case(small, "probe_keys", placed=False)
    try:
        keys = small.t.bits["g"][idx]
        assert len(idx) == 512 and 2 * len(idx) <= 1024                     # ws_group_by sizes the table at 1024 slots
        with np.errstate(over="ignore"):
            home = _key_slot(np.unique(keys))
        assert len(home) == 256 and home.min() >= 1016 and home.max() <= 1023
        cols, _ = _check(small, rows, idx, ["g"], [("COUNT", None), ("SUM", "v"), ("MAX", "v")], "probe chain")
        assert len(cols[0]) == 256 and (cols[1] == 2).all()
    finally:
        rows.free()


def test_probe_chain_wraps_distinct_table(small):
    """The same for k_gb_distinct's table: one group (a constant key), 256 values, each twice."""
    rows, idx = _case(small, "probe_distinct", placed=False)
    try:
        vals = small.t.bits["v"][idx]
        with np.errstate(over="ignore"):
            home = _distinct_slot(np.unique(vals))
        assert len(idx) == 512 and len(home) == 256 and home.min() >= 1016 and home.max() <= 1023
        cols, _ = _check(small, rows, idx, [], [("COUNT", None), ("COUNT_DISTINCT", "v"), ("SUM", "v")], "distinct chain")
        assert cols[0][0] == 512 and cols[1][0] == 256
    finally:
        rows.free()
