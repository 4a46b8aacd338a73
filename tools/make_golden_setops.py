#!/usr/bin/env python3
"""Regenerate tests/golden/setop_golden.json from the reference's own src/graph/test/SetTest.cpp
(run where the reference checkout is; NEBULA_REF names it).

Extracted (data only — query text with the vids resolved, expected status, column names, expected
rows): every `{ cpp2::ExecutionResponse resp; ... }` block of every SetTest case, the way
tools/make_golden_orderby.py does it.  A block that asserts no rows (`ASSERT_EQ(nullptr,
resp.get_rows())`) records only what it asserts: "no_rows"; so does a block that fills `expected`
but never compares it (status and column names only).  SetTest builds its expected rows by
looping over the data set (`for (auto &serve : tim.serves()) { ... expected.emplace_back(...) }`);
expected_rows() below evaluates those loops over tools/make_golden.py's parse of the same data
set, so the file holds the rows themselves.  Cases that cannot be expressed are recorded under
"skipped" with the reason.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import make_golden_groupby as mgg  # noqa: E402
import make_golden_orderby as mgo  # noqa: E402

SOURCE = "src/graph/test/SetTest.cpp"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "setop_golden.json")


def matching_brace(text, i):
    """Index just past the `}` closing the `{` at text[i]."""
    depth, j = 1, i + 1
    while depth:
        depth += (text[j] == "{") - (text[j] == "}")
        j += 1
    return j


class Continue(Exception):
    pass


def run_stmts(data, text, env, out):
    """The statements SetTest uses to fill `expected`: range-for over serves() / likes(), a player
    looked up by a like's name, `if (a.name() == b.name()) { continue; }`, and a tuple record
    appended.  env: variable -> player name, or a serve (team, start, end) / like (name, likeness)."""
    def value(e):
        e = e.strip()
        m = re.fullmatch(r"folly::to<std::string>\((.*)\)", e, re.S)
        if m:
            return str(value(m.group(1)))
        m = re.fullmatch(r"(\w+)\.name\(\)", e)
        if m:
            return env[m.group(1)]
        m = re.fullmatch(r"std::get<(\d)>\((\w+)\)", e)
        if m:
            return env[m.group(2)][int(m.group(1))]
        raise ValueError("expression " + e)

    i = 0
    while i < len(text):
        rest = text[i:]
        m = re.match(r"\s*for \(auto &(\w+) : (\w+)\.(serves|likes)\(\)\) \{", rest)
        if m:
            end = matching_brace(text, i + m.end() - 1)
            who = env[m.group(2)]
            items = [tuple(r[1:]) for r in data["serve" if m.group(3) == "serves" else "like"] if r[0] == who]
            for it in items:
                try:
                    run_stmts(data, text[i + m.end():end - 1], {**env, m.group(1): it}, out)
                except Continue:
                    pass
            i = end
            continue
        m = re.match(r"\s*auto &(\w+) = players_\[std::get<0>\((\w+)\)\];", rest)
        if m:
            env = {**env, m.group(1): env[m.group(2)][0]}
            i += m.end()
            continue
        m = re.match(r"\s*if \((\w+)\.name\(\) == (\w+)\.name\(\)\) \{\s*continue;\s*\}", rest)
        if m:
            if env[m.group(1)] == env[m.group(2)]:
                raise Continue()
            i += m.end()
            continue
        m = re.match(r"\s*std::tuple<[^;]*?>\s*record\((.*?)\);\s*expected\.emplace_back\(std::move\(record\)\);", rest, re.S)
        if m:
            args, depth, cur = [], 0, ""
            for ch in m.group(1):
                if ch == "," and depth == 0:
                    args.append(cur)
                    cur = ""
                    continue
                depth += (ch in "(<") - (ch in ")>")
                cur += ch
            out.append([value(a) for a in args + [cur]])
            i += m.end()
            continue
        if not rest.strip():
            break
        raise ValueError("statement near " + rest[:60])


def expected_rows(ctx, data, block):
    m = re.search(r"std::vector<std::tuple<[^;]*>>\s*expected;(.*?)ASSERT_TRUE\(verifyResult\(resp, expected\)\);", block, re.S)
    if not m:
        return None
    out = []
    run_stmts(data, m.group(1), dict(ctx.vars), out)
    return out


def parse_case(ctx, data, name, block):
    case = mgg.parse_case(ctx, name, block)
    case["source"] = SOURCE
    if case["status"] == "SUCCEEDED" and "expected" not in case:
        rows = expected_rows(ctx, data, block)
        if rows is not None:
            case["expected"] = rows
    m = re.search(r"colsExpect = \{(.*?)\};", block)
    if m:
        case["col_names"] = mg.scan_init(ctx, m.group(1))
    if case["status"] == "SUCCEEDED" and re.search(r"ASSERT_EQ\(nullptr, resp\.get_rows\(\)\)", block):
        case.pop("expected", None)
        case["no_rows"] = True
    return case


def main():
    data = mg.parse_dataset()
    ctx = mgg.Ctx(data)
    cases, skipped = [], []
    for name, body in mgo.test_bodies(mg.read(SOURCE), "SetTest"):
        for block in mgo.case_blocks(body):
            case = parse_case(ctx, data, name, block)
            judged = case["status"] != "SUCCEEDED" or "expected" in case or case.get("no_rows") or "col_names" in case
            if not case["query"] or not judged:
                skipped.append({"test": case["test"], "query": case["query"], "reason": "no query text or no expectation found"})
            else:
                cases.append(case)
    with open(OUT, "w") as f:
        json.dump({"sources": [SOURCE], "cases": cases, "skipped": skipped}, f, indent=1)
        f.write("\n")
    print(f"setop cases={len(cases)} skipped={len(skipped)}")


if __name__ == "__main__":
    main()
