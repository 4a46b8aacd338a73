#!/usr/bin/env python3
"""Regenerate tests/golden/groupby_golden.json from the reference's own
src/graph/test/GroupByLimitTest.cpp (run where the reference checkout is; NEBULA_REF names it).

Extracted (data only — query text, expected status, column names, expected rows): the cases
whose pipeline consists of GO and GROUP BY only, i.e. every GroupByTest case (its
`| GO FROM $-.id` "Output next" case included) and every SyntaxError case that contains GROUP BY.
Player names are resolved to vids as tools/make_golden.py does.  Expected values take the C++
tuple's declared types (a `double` column written `0` is 0.0).  The cases left out (ORDER BY /
LIMIT pipelines, statements without GROUP BY) are recorded under "skipped" with the reason.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

SOURCE = "src/graph/test/GroupByLimitTest.cpp"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "groupby_golden.json")

# make_golden's literal scanner plus floating-point literals
TOK = re.compile(r'''\s*(?:(?P<str>"(?:[^"\\]|\\.)*")|(?P<dbl>-?\d+\.\d*)|(?P<num>-?\d+)|(?P<open>\{)|(?P<close>\})
                     |(?P<comma>,)
                     |(?P<ref>(?:players_|teams_)\["[^"]+"\]\.(?:vid|name)\(\))
                     |(?P<var>[A-Za-z_]\w*\.(?:vid|name)\(\))
                     |(?P<ident>[A-Za-z_]\w*))''', re.X)


class Ctx(mg.Ctx):
    def value(self, kind, text):
        if kind == "dbl":
            return float(text)
        return super().value(kind, text)


def tuple_types(block):
    """Python constructors for the columns of `std::vector<std::tuple<...>> expected`."""
    m = re.search(r"std::vector<\s*std::tuple<(.*?)>\s*>\s*expected", re.sub(r"//[^\n]*", "", block), re.S)
    if not m:
        return None
    body = m.group(1)
    out = []
    for t in body.split(","):
        t = t.strip()
        if t:
            out.append(float if t == "double" else str if t == "std::string" else int)
    return out


def parse_case(ctx, name, block):
    mg.TOK = TOK
    case = mg.parse_block(ctx, block)
    case = {"test": name, "source": SOURCE, "query": case["query"],
            **{k: v for k, v in case.items() if k in ("col_names", "expected")}}
    m = re.search(r"ASSERT_EQ\(cpp2::ErrorCode::(\w+), code\)", block)
    case["status"] = m.group(1)
    types = tuple_types(block)
    if types and "expected" in case:
        case["expected"] = [[t(v) for t, v in zip(types, row)] for row in case["expected"]]
    if case["status"] != "SUCCEEDED":
        case.pop("expected", None)
    return case


def main():
    data = mg.parse_dataset()
    ctx = Ctx(data)
    cases, skipped = [], []
    for name, block in mg.blocks(mg.read(SOURCE), "GroupByLimitTest"):
        case = parse_case(ctx, name, block)
        q = case["query"] or ""
        why = None
        if re.search(r"\bORDER BY\b|\bLIMIT\b", q):
            why = "the pipeline has ORDER BY / LIMIT"
        elif "GROUP BY" not in q:
            why = "no GROUP BY in the statement"
        elif name not in ("GroupByTest", "SyntaxError"):
            why = "not a GroupByTest / SyntaxError case"
        if why:
            skipped.append({"test": name, "query": q, "reason": why})
        else:
            cases.append(case)
    with open(OUT, "w") as f:
        json.dump({"source": SOURCE, "cases": cases, "skipped": skipped}, f, indent=1)
        f.write("\n")
    print(f"groupby cases={len(cases)} skipped={len(skipped)}")


if __name__ == "__main__":
    main()
