#!/usr/bin/env python3
"""Regenerate tests/golden/fetch_edges_golden.json from the reference's own
src/graph/test/FetchEdgesTest.cpp (run where the reference checkout is; NEBULA_REF names it).

Extracted (data only — query text with the vids resolved, expected status, expected column names
and rows): every `{ cpp2::ExecutionResponse resp; ... }` block of the base, noYield, distinct,
noInput, syntaxError and nonExistEdge cases, the way tools/make_golden_fetch.py does it.  The
test's C++ reads its expectations from the data set (`player.serves()[k]`, `std::get<1>(serve)`,
`teams_[std::get<0>(serve)]`, a loop over `player.serves()`); resolve_serves() below looks those up
in tools/make_golden.py's parse of the same data set, so the file holds the rows themselves.  The
`uuid(...)` blocks need the meta service to hand out ids; they are recorded under "skipped" with
the reason.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import make_golden as mg  # noqa: E402
import make_golden_fetch as mgf  # noqa: E402
import make_golden_groupby as mgg  # noqa: E402
import make_golden_orderby as mgo  # noqa: E402

SOURCE = "src/graph/test/FetchEdgesTest.cpp"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "fetch_edges_golden.json")
TESTS = ("base", "noYield", "distinct", "noInput", "syntaxError", "nonExistEdge")


def resolve_serves(data, block):
    """`auto &s = p.serves()[k]`, `teams_[std::get<0>(s)]`, `std::get<1|2>(s)` and the loop that
    fills `expected` from `p.serves()` become literals, so mg.parse_block reads plain initialisers."""
    who = dict(re.findall(r'auto\s*&\s*(\w+)\s*=\s*players_\["([^"]+)"\]\s*;', block))
    serves_of = {}
    for w, team, start, end in data["serve"]:
        serves_of.setdefault(w, []).append((team, start, end))
    serve = {}
    for var, p, k in re.findall(r"auto\s*&\s*(\w+)\s*=\s*(\w+)\.serves\(\)\[(\d+)\]\s*;", block):
        serve[var] = serves_of[who[p]][int(k)]
    block = re.sub(r"teams_\[std::get<0>\((\w+)\)\]", lambda m: 'teams_["%s"]' % serve[m.group(1)][0], block)
    block = re.sub(r"std::get<([12])>\((\w+)\)", lambda m: str(serve[m.group(2)][int(m.group(1))]) if m.group(2) in serve else m.group(0), block)

    def loop(m):
        rows = ", ".join("{%d, %d}" % (s, e) for _, s, e in serves_of[who[m.group(2)]])
        return "%s expected = {%s};" % (m.group(1), rows)
    block = re.sub(r"(std::vector<std::tuple<int64_t, int64_t>>) expected;\s*for \(auto &serve : (\w+)\.serves\(\)\) \{.*?\n        \}",
                   loop, block, flags=re.S)
    block = block.replace(".c_str()", "").replace("%s", "%ld")   # (mg.printf_ld fills %ld with str(arg))
    return re.sub(r"(\d+)\s*>\s*(\d+),", lambda m: str(int(int(m.group(1)) > int(m.group(2)))) + ",", block)


def main():
    data = mg.parse_dataset()
    ctx = mgg.Ctx(data)
    cases, skipped = [], []
    for name, body in mgo.test_bodies(mg.read(SOURCE), "FetchEdgesTest"):
        if name not in TESTS:
            continue
        for block in mgf.case_blocks(body, None):
            if "uuid(" in block:
                q = re.search(r'auto (?:\*fmt|query) = ((?:"(?:[^"\\]|\\.)*"\s*)+);', block)
                skipped.append({"test": name, "query": mg.cpp_strings(q.group(1)) if q else "",
                                "reason": "uuid() asks the meta service for an id; there is none here"})
                continue
            block = resolve_serves(data, block)
            case = mgg.parse_case(ctx, name, block)
            case["source"] = SOURCE
            mgf.bool_columns(block, case)
            if not case["query"] or (case["status"] == "SUCCEEDED" and "expected" not in case):
                skipped.append({"test": name, "query": case["query"], "reason": "no query text or no expectation found"})
            else:
                cases.append(case)
    with open(OUT, "w") as f:
        json.dump({"sources": [SOURCE], "cases": cases, "skipped": skipped}, f, indent=1)
        f.write("\n")
    print(f"fetch edges cases={len(cases)} skipped={len(skipped)}")


if __name__ == "__main__":
    main()
