"""Pins the GROUP BY checker (tests/support/groupby.py: parser, model, session) to the reference's
own GroupByLimitTest vectors before it judges the device: over the CPU oracle's GO rows the model
reproduces every case of tests/golden/groupby_golden.json — statuses, column names where the
reference asserts them, rows as multisets.  CPU only."""
import pytest

from tests.support import golden, groupby
from tests.support.oracle import nba_oracle

GOLDEN = golden.load("groupby_golden.json")
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def orc(nba_data):
    o = nba_oracle(nba_data)
    yield o
    o.close()


def test_golden_file_shape():
    assert len(CASES) == 15
    assert sum(c["status"] == "SUCCEEDED" for c in CASES) == 6
    assert all("GROUP BY" in c["query"] for c in CASES)
    assert GOLDEN["skipped"] and all(s["reason"] for s in GOLDEN["skipped"])


@pytest.mark.parametrize("case", CASES, ids=[f"{c['test']}-{i}" for i, c in enumerate(CASES)])
def test_model_reproduces_golden(orc, case):
    ok, msg = groupby.run_case(groupby.Session(orc), case)
    assert ok, msg


def test_split_pipes():
    assert groupby.split_pipes("GO FROM 1 OVER e WHERE e.w > 1 || e.w < 0 | GROUP BY $-.a YIELD COUNT(*)") == \
        ["GO FROM 1 OVER e WHERE e.w > 1 || e.w < 0 ", " GROUP BY $-.a YIELD COUNT(*)"]
    assert groupby.split_pipes('GO FROM 1 OVER e YIELD "a|b" AS s') == ['GO FROM 1 OVER e YIELD "a|b" AS s']


def test_model_functions_by_type():
    """nbg.h "Functions": the type decides (SUM over BOOL is INT 0, AVG over STRING 0.0, STD over a
    VID INT 0, bit folds over INT only), -0.0 and 0.0 are one key, MAX / MIN keep the column's order."""
    from tests.support.ngql import Interim
    inp = Interim(["k", "i", "d", "b", "s", "v"],
                  [[0.0, -5, -1.5, True, "b", 7], [-0.0, 3, 2.25, False, "a", 9], [1.0, 1 << 62, 0.5, True, "c", 1]])
    types = ["DOUBLE", "INT", "DOUBLE", "BOOL", "STRING", "VID"]
    p = groupby.parse_sentence(
        "GROUP BY $-.k YIELD COUNT(*), SUM($-.i), SUM($-.d), SUM($-.b), AVG($-.s), MAX($-.d), MIN($-.i), MAX($-.b), "
        "MIN($-.s), STD($-.v), STD($-.i), BIT_XOR($-.i), BIT_AND($-.d), COUNT_DISTINCT($-.b), SUM($-.v)")
    out = groupby.group_model(inp, p.groups, p.yields, types)
    rows = sorted(out.rows)
    assert rows[0] == [1, 1 << 62, 0.5, 0, 0.0, 0.5, 1 << 62, True, "c", 0, 0.0, 1 << 62, 0, 1, 1]
    assert rows[1] == [2, -2, 0.75, 0, 0.0, 2.25, -5, True, "a", 0, 4.0, -5 ^ 3, 0, 2, 16]
