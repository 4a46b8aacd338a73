#!/usr/bin/env python3
"""Regenerate tests/golden/fetch_golden.json from the reference's own
src/graph/test/FetchVerticesTest.cpp (run where the reference checkout is; NEBULA_REF names it).

Extracted (data only — query text with the vids resolved, expected status, expected column names
and rows): every `{ cpp2::ExecutionResponse resp; ... }` block of the base, noYield, distinct,
syntaxError, executionError and nonExistVertex cases, the way tools/make_golden_yield.py does it.
nonExistVertex computes its vid (`std::hash<std::string>()("NON EXIST VERTEX ID")`, bumped past
every player's vid); non_exist_vid() below restates that loop over tools/make_golden.py's parse of
the same data set.  `player.age()` and `player.age() > 30` in an expected tuple are looked up and
evaluated here, so the file holds the rows themselves.  The `uuid(...)` blocks need the meta
service to hand out ids; they are recorded under "skipped" with the reason.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import make_golden as mg  # noqa: E402
import make_golden_groupby as mgg  # noqa: E402
import make_golden_orderby as mgo  # noqa: E402
from nebula_amd.vidhash import std_hash  # noqa: E402

SOURCE = "src/graph/test/FetchVerticesTest.cpp"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "fetch_golden.json")
TESTS = ("base", "noYield", "distinct", "syntaxError", "executionError", "nonExistVertex")


def non_exist_vid(data, body):
    name = re.search(r'std::string name = "([^"]+)";', body).group(1)
    vid = std_hash(name)
    vids = {p["vid"] for p in data["players"]}
    while vid in vids:
        vid += 1
    return vid


def case_blocks(body, vid):
    """The blocks of one TEST_F; `player.age() > 30` becomes its value's spelling and
    nonExistPlayerID its number, so mg.parse_block reads plain initialisers."""
    for b in re.split(r"\n\s*\{\s*\n\s*cpp2::ExecutionResponse resp;", body)[1:]:
        if vid is not None:
            b = b.replace("nonExistPlayerID", str(vid))
        yield b


def resolve_ages(data, block):
    """`<who>.age()` and `players_["X"].age()` become the number and `<age> > N` its truth value
    (1 / 0; bool_columns() turns those cells back into bools), so mg.parse_block reads literals."""
    age = {p["name"]: p["age"] for p in data["players"]}
    block = block.replace(".c_str()", "").replace("%s", "%ld")   # (mg.printf_ld fills %ld with str(arg))
    who = dict(re.findall(r'auto\s*&\s*(\w+)\s*=\s*players_\["([^"]+)"\]\s*;', block))
    block = re.sub(r'players_\["([^"]+)"\]\.age\(\)', lambda m: str(age[m.group(1)]), block)
    block = re.sub(r"\b(\w+)\.age\(\)", lambda m: str(age[who[m.group(1)]]), block)
    return re.sub(r"(\d+)\s*>\s*(\d+)\}", lambda m: str(int(int(m.group(1)) > int(m.group(2)))) + "}", block)


def bool_columns(block, case):
    m = re.search(r"std::vector<\s*std::tuple<(.*?)>\s*>\s*expected", block, re.S)
    if not m or "expected" not in case:
        return
    for k, t in enumerate(x.strip() for x in m.group(1).split(",")):
        if t == "bool":
            for r in case["expected"]:
                r[k] = bool(r[k])


def main():
    data = mg.parse_dataset()
    ctx = mgg.Ctx(data)
    cases, skipped = [], []
    for name, body in mgo.test_bodies(mg.read(SOURCE), "FetchVerticesTest"):
        if name not in TESTS:
            continue
        vid = non_exist_vid(data, body) if name == "nonExistVertex" else None
        for block in case_blocks(body, vid):
            if "uuid(" in block:
                q = re.search(r'auto \*fmt = ((?:"(?:[^"\\]|\\.)*"\s*)+);', block)
                skipped.append({"test": name, "query": mg.cpp_strings(q.group(1)) if q else "",
                                "reason": "uuid() asks the meta service for an id; there is none here"})
                continue
            block = resolve_ages(data, block)
            case = mgg.parse_case(ctx, name, block)
            case["source"] = SOURCE
            bool_columns(block, case)
            if not case["query"] or (case["status"] == "SUCCEEDED" and "expected" not in case):
                skipped.append({"test": name, "query": case["query"], "reason": "no query text or no expectation found"})
            else:
                if "verifyResult(resp, expected, false)" in block:
                    case["ordered"] = True
                cases.append(case)
    with open(OUT, "w") as f:
        json.dump({"sources": [SOURCE], "cases": cases, "skipped": skipped}, f, indent=1)
        f.write("\n")
    print(f"fetch cases={len(cases)} skipped={len(skipped)}")


if __name__ == "__main__":
    main()
