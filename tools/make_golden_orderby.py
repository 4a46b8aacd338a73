#!/usr/bin/env python3
"""Regenerate tests/golden/orderby_golden.json from the reference's own
src/graph/test/OrderByTest.cpp and src/graph/test/GroupByLimitTest.cpp (run where the reference
checkout is; NEBULA_REF names it).

Extracted (data only — query text, expected status, column names, expected rows): every
OrderByTest case, and every GroupByLimitTest case whose pipeline has ORDER BY or LIMIT (the ones
tests/golden/groupby_golden.json lists as skipped for that reason, the two `LIMIT -1, 2` /
`LIMIT 1, -2` syntax cases included).  Player names are resolved to vids as tools/make_golden.py
does; expected values take the C++ tuple's declared types.  Per case:
  ordered    the rows are compared in the listed order: verifyResult's third argument (sortEnable)
             is `false`; without it both sides are sorted first
  match      false where the reference asserts that the listed rows are NOT the result
             (ASSERT_FALSE(verifyResult(...)), OrderByTest.SingleFactor)
  row_count  where the reference asserts only the number of rows
A block that runs a second query against the same expectation (`fmt1`) gives a second case.
Cases that cannot be expressed are recorded under "skipped" with the reason.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import make_golden_groupby as mgg  # noqa: E402

ORDER_SOURCE = "src/graph/test/OrderByTest.cpp"
LIMIT_SOURCE = "src/graph/test/GroupByLimitTest.cpp"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "orderby_golden.json")
LITERALS = r'((?:"(?:[^"\\]|\\.)*"\s*)+)'


def test_bodies(src, cls):
    """(test name, body text) of every TEST_F of `cls`."""
    for t in re.finditer(r"TEST_F\(%s, (\w+)\)\s*\{" % cls, src):
        depth, i = 1, t.end()
        while depth:
            depth += (src[i] == "{") - (src[i] == "}")
            i += 1
        yield t.group(1), src[t.end():i - 1]


def case_blocks(body):
    """The `{ cpp2::ExecutionResponse resp; ... }` blocks of a test body, with the test's shared
    `std::string go = "..."` prefix written back into each block's `auto fmt = go + "..."`."""
    go = re.search(r"std::string go\s*=\s*" + LITERALS + ";", body)
    for b in re.split(r"\n\s*\{\s*\n\s*cpp2::ExecutionResponse resp;", body)[1:]:
        if go:
            b = b.replace("auto fmt = go + ", "auto *fmt = " + go.group(1) + " ").replace("fmt.c_str()", "fmt")
        yield b


def parse_case(ctx, name, source, block):
    case = mgg.parse_case(ctx, name, block)
    case["source"] = source
    if case["status"] == "SUCCEEDED":
        m = re.search(r"ASSERT_(TRUE|FALSE)\(verifyResult\(resp, expected(?:,\s*(\w+))?\)\)", block)
        if m:
            case["ordered"] = m.group(2) == "false"
            if m.group(1) == "FALSE":
                case["match"] = False
        m = re.search(r"ASSERT_EQ\((\d+), resp\.get_rows\(\)->size\(\)\)", block)
        if m:
            case["row_count"] = int(m.group(1))
    cases = [case]
    m = re.search(r"auto\s*\*\s*fmt1\s*=\s*" + LITERALS + r";\s*query = folly::stringPrintf\(\s*fmt1\s*,(.*?)\);", block, re.S)
    if m:   # a second query judged by the same expectation
        again = dict(case)
        again["query"] = mg.printf_ld(mg.cpp_strings(m.group(1)), mg.scan_init(ctx, m.group(2)))
        cases.append(again)
    return cases


def main():
    ctx = mgg.Ctx(mg.parse_dataset())
    cases, skipped = [], []
    for name, body in test_bodies(mg.read(ORDER_SOURCE), "OrderByTest"):
        for block in case_blocks(body):
            cases.extend(parse_case(ctx, name, ORDER_SOURCE, block))
    for name, body in test_bodies(mg.read(LIMIT_SOURCE), "GroupByLimitTest"):
        for block in case_blocks(body):
            for case in parse_case(ctx, name, LIMIT_SOURCE, block):
                if re.search(r"\bORDER BY\b|\bLIMIT\b", case["query"] or ""):
                    cases.append(case)
    for case in list(cases):
        judged = case["status"] != "SUCCEEDED" or "expected" in case or "row_count" in case
        if not case["query"] or not judged:
            cases.remove(case)
            skipped.append({"test": case["test"], "query": case["query"], "reason": "no query text or no expectation found"})
    with open(OUT, "w") as f:
        json.dump({"sources": [ORDER_SOURCE, LIMIT_SOURCE], "cases": cases, "skipped": skipped}, f, indent=1)
        f.write("\n")
    print(f"orderby cases={len(cases)} skipped={len(skipped)}")


if __name__ == "__main__":
    main()
