#!/usr/bin/env python3
"""Regenerate tests/golden/yield_golden.json from the reference's own src/graph/test/YieldTest.cpp
(run where the reference checkout is; NEBULA_REF names it).

Extracted (data only — query text with the vids resolved, expected status, expected rows): every
`{ cpp2::ExecutionResponse resp; ... }` block of the yieldPipe, yieldVar, error and AggCall cases,
the way tools/make_golden_setops.py does it.  The other YieldTest cases (basic, hashCall, Logic,
inCall) are constant YIELDs without input; tests/golden/expression_cases.json already holds them.
YieldTest builds most expected rows by looping over the data set (`for (auto &serve :
player.serves()) { if (std::get<1>(serve) <= 2005) { continue; } ... expected.emplace_back(...) }`);
expected_rows() below evaluates those loops over tools/make_golden.py's parse of the same data
set, so the file holds the rows themselves.  A block that asserts no status (`yield $-`) is
recorded under "skipped" with the reason.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import make_golden_groupby as mgg  # noqa: E402
import make_golden_orderby as mgo  # noqa: E402
import make_golden_setops as mgs  # noqa: E402

SOURCE = "src/graph/test/YieldTest.cpp"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "yield_golden.json")
TESTS = ("yieldPipe", "yieldVar", "error", "AggCall")


def case_blocks(body):
    """mgo.case_blocks for YieldTest's spellings: the shared prefix is `std::string go` or
    `std::string var`, a block may declare `std::string fmt`, and `expected{...}` initialises."""
    prefix = re.search(r"std::string (go|var)\s*=\s*" + mgo.LITERALS + ";", body)
    for b in re.split(r"\n\s*\{\s*\n\s*cpp2::ExecutionResponse resp;", body)[1:]:
        if prefix:
            b = b.replace("auto fmt = %s + " % prefix.group(1), "auto *fmt = " + prefix.group(2) + " ")
        b = b.replace("std::string fmt = ", "auto *fmt = ").replace("fmt.c_str()", "fmt")
        b = re.sub(r"(>\s*expected)\s*\{", r"\1 = {", b)
        yield b


def run_stmts(data, text, env, out):
    """The statements YieldTest uses to fill `expected`: a range-for over serves(), `if
    (std::get<N>(serve) <= K) { continue; }`, and a tuple `result` appended."""
    def value(e):
        e = e.strip()
        m = re.fullmatch(r"(\w+)\.name\(\)", e)
        if m:
            return env[m.group(1)]
        m = re.fullmatch(r"std::get<(\d)>\((\w+)\)", e)
        if m:
            return env[m.group(2)][int(m.group(1))]
        m = re.fullmatch(r"std::hash<int32_t>\{\}\((-?\d+)\)", e)   # (the identity on an int32)
        if m:
            return int(m.group(1))
        raise ValueError("expression " + e)

    i = 0
    while i < len(text):
        rest = text[i:]
        m = re.match(r"\s*for \(auto &(\w+) : (\w+)\.serves\(\)\) \{", rest)
        if m:
            end = mgs.matching_brace(text, i + m.end() - 1)
            who = env[m.group(2)]
            for it in [tuple(r[1:]) for r in data["serve"] if r[0] == who]:
                try:
                    run_stmts(data, text[i + m.end():end - 1], {**env, m.group(1): it}, out)
                except mgs.Continue:
                    pass
            i = end
            continue
        m = re.match(r"\s*if \(std::get<(\d)>\((\w+)\) <= (-?\d+)\) \{\s*continue;\s*\}", rest)
        if m:
            if env[m.group(2)][int(m.group(1))] <= int(m.group(3)):
                raise mgs.Continue()
            i += m.end()
            continue
        m = re.match(r"\s*std::tuple<[^;]*?>\s*result\((.*?)\);\s*expected\.emplace_back\(std::move\(result\)\);", rest, re.S)
        if m:
            args, depth, cur = [], 0, ""
            for ch in m.group(1):
                if ch == "," and depth == 0:
                    args.append(cur)
                    cur = ""
                    continue
                depth += (ch in "(<{") - (ch in ")>}")
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


def main():
    data = mg.parse_dataset()
    ctx = mgg.Ctx(data)
    cases, skipped = [], []
    for name, body in mgo.test_bodies(mg.read(SOURCE), "YieldTest"):
        if name not in TESTS:
            continue
        for block in case_blocks(body):
            if not re.search(r"ASSERT_EQ\(cpp2::ErrorCode::(\w+), code\)", block):
                q = mg.parse_block(ctx, block)["query"]
                skipped.append({"test": name, "query": q, "reason": "the reference asserts no status for it"})
                continue
            case = mgg.parse_case(ctx, name, block)
            case["source"] = SOURCE
            if case["status"] == "SUCCEEDED" and "expected" not in case:
                rows = expected_rows(ctx, data, block)
                if rows is not None:
                    case["expected"] = rows
            if not case["query"] or (case["status"] == "SUCCEEDED" and "expected" not in case):
                skipped.append({"test": name, "query": case["query"], "reason": "no query text or no expectation found"})
            else:
                cases.append(case)
    with open(OUT, "w") as f:
        json.dump({"sources": [SOURCE], "cases": cases, "skipped": skipped}, f, indent=1)
        f.write("\n")
    print(f"yield cases={len(cases)} skipped={len(skipped)}")


if __name__ == "__main__":
    main()
