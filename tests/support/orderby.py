"""TEST HARNESS: `| ORDER BY ...` and `| LIMIT ...` for the nGQL front end of tests/support/ngql.py
and groupby.py, a plain-Python model of OrderByExecutor (src/graph/OrderByExecutor.cpp:94-155) and
LimitExecutor (src/graph/LimitExecutor.cpp:18-66) as include/nbg.h restates them for nbg_order_by,
and a session whose device mode keeps a whole `GO | GROUP BY | ORDER BY | LIMIT` pipeline in HBM.

The model is the checker of tests/test_gpu_orderby.py; tests/test_orderby_model.py pins it to the
reference's own OrderByTest / GroupByLimitTest vectors (tests/golden/orderby_golden.json) first.

`LIMIT a OFFSET b` is `LIMIT a, b` in the reference's grammar (parser.yy:872-876: both build
LimitSentence($2, $4), i.e. offset a and count b), which is what its LimitTest expects.
"""
from __future__ import annotations

import functools
from collections import Counter
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from nebula_amd import _lib
from tests.support import groupby, ngql
from tests.support.groupby import GroupBySentence, GroupError

INT64_MAX = (1 << 63) - 1


@dataclass
class OrderBySentence:
    factors: List[Tuple[str, bool]] = field(default_factory=list)    # (column name, descending)


@dataclass
class LimitSentence:
    offset: int = 0
    count: int = 0


STAGES = (GroupBySentence, OrderBySentence, LimitSentence)


class Parser(groupby.Parser):
    """groupby.Parser plus order_by_sentence (parser.yy:727-767: `$-.name` or a bare label, optional
    ASC / DESC) and limit_sentence (:872-876)."""

    def primary_sentence(self):
        if self.kw("ORDER"):
            return self.order_by()
        if self.kw("LIMIT"):
            return self.limit()
        return super().primary_sentence()

    def order_by(self):
        self.expect_kw("ORDER")
        self.expect_kw("BY")
        s = OrderBySentence([self.order_factor()])
        while self.sym(","):
            self.take()
            s.factors.append(self.order_factor())
        return s

    def order_factor(self):
        if self.sym("$-"):
            self.take()
            self.expect_sym(".")
        kind, name = self.take()
        if kind != "name":
            raise ngql.ParseError(f"expected a column name near {name!r}")
        desc = False
        if self.kw("ASC", "DESC"):
            desc = self.take()[1].upper() == "DESC"
        return name, desc

    def integer(self):
        # (the scanner has no negative INTEGER: `LIMIT -1, 2` is a syntax error either way; the
        # sign is kept so that the prepare check of LimitExecutor answers it)
        neg = False
        if self.sym("-"):
            self.take()
            neg = True
        kind, text = self.take()
        if kind != "int":
            raise ngql.ParseError(f"expected an integer near {text!r}")
        v = ngql.int_literal(text)
        return -v if neg else v

    def limit(self):
        self.expect_kw("LIMIT")
        a = self.integer()
        if self.sym(",") or self.kw("OFFSET"):
            self.take()
            return LimitSentence(a, self.integer())
        return LimitSentence(0, a)


def parse_sentence(text: str):
    p = Parser(text)
    s = p.primary_sentence()
    if p.peek()[0] != "eof":
        raise ngql.ParseError(f"trailing input near {p.peek()[1]!r}")
    return s


# ------------------------------------------------------------------------------------ the model
def check_limit(offset: int, count: int):
    """LimitExecutor::prepare."""
    if offset < 0:
        raise GroupError(_lib.E_SYNTAX_ERROR, f"skip `{offset}' is illegal")
    if count < 0:
        raise GroupError(_lib.E_SYNTAX_ERROR, f"count `{count}' is illegal")


def window(rows: int, offset: int, count: int):
    """The [lo, hi) a LIMIT keeps of `rows` rows (offset + count saturates)."""
    if count == 0 or rows <= offset:
        return 0, 0
    return offset, min(rows, min(offset + count, INT64_MAX))


def factor_columns(columns, factors):
    """getFieldIndex per factor: the first column of that name, else E_EXECUTION_ERROR."""
    out = []
    for name, _ in factors:
        if name not in columns:
            raise GroupError(_lib.E_EXECUTION_ERROR, f"Field ({name}) not exist in input schema.")
        out.append(columns.index(name))
    return out


def order_model(inp: ngql.Interim, factors) -> ngql.Interim:
    """OrderByExecutor over an Interim: ColumnValue::operator< per factor, -0.0 == 0.0 (Python's
    == and < on floats are IEEE's), later factors breaking ties."""
    if not inp.rows:                      # beforeExecute returns before the factor check
        return ngql.Interim(inp.columns, [])
    cols = factor_columns(inp.columns, factors)

    def cmp(a, b):
        for c, (_, desc) in zip(cols, factors):
            if a[c] == b[c]:
                continue
            less = a[c] < b[c]
            return -1 if less != desc else 1
        return 0
    return ngql.Interim(inp.columns, sorted(inp.rows, key=functools.cmp_to_key(cmp)))


def limit_model(inp: ngql.Interim, offset: int, count: int) -> ngql.Interim:
    check_limit(offset, count)
    lo, hi = window(len(inp.rows), offset, count)
    return ngql.Interim(inp.columns, inp.rows[lo:hi])


# ------------------------------------------------------------------------------------ execution
class Session(groupby.Session):
    """groupby.Session plus ORDER BY and LIMIT.  In device mode a GO followed by any run of
    GROUP BY / ORDER BY / LIMIT stages stays on the device: go_device, then Engine.group_by /
    Engine.order_by per stage (an adjacent `ORDER BY | LIMIT` is one call), one fetch at the end of
    the run — the end of the statement or a following `| GO FROM $-.id`."""

    def execute(self, text: str) -> ngql.Interim:
        sents = [parse_sentence(p) for p in groupby.split_pipes(text)]
        for st in sents:                  # every executor's prepare() runs before the first execute()
            if isinstance(st, LimitSentence):
                check_limit(st.offset, st.count)
        result, i = None, 0
        while i < len(sents):
            st = sents[i]
            if self.device and isinstance(st, ngql.GoSentence) and i + 1 < len(sents) and isinstance(sents[i + 1], STAGES):
                j = i + 1
                while j < len(sents) and isinstance(sents[j], STAGES):
                    j += 1
                result = self._go_stages_device(st, sents[i + 1:j], result)
                i = j
                continue
            result = self._run(st, result)
            i += 1
        return result if result is not None else ngql.Interim([], [])

    def _run(self, st, inp):
        if isinstance(st, OrderBySentence):
            return order_model(inp, st.factors) if inp is not None else ngql.Interim([], [])
        if isinstance(st, LimitSentence):
            return limit_model(inp, st.offset, st.count) if inp is not None else ngql.Interim([], [])
        r = super()._run(st, inp)
        if isinstance(st, GroupBySentence):
            self.last_types = None        # (a later stage types the aggregates by their values)
        return r

    def _go_stages_device(self, g: ngql.GoSentence, stages, inp):
        if g.upto or g.reversely or g.over_all or g.yields is None:
            raise ngql.ExecError("device pipeline harness: GO needs OVER names and a YIELD")
        etypes = self._edge_types(g.over, False)
        names = [c.name() for c in g.yields]
        if g.from_ref is not None:
            src = self._source(g.from_ref, inp)
            starts = [int(v) for v in src.col(g.from_ref[1])] if src is not None and src.rows else []
        else:
            starts = list(g.from_vids)
        rows = self.b.go_device(starts, etypes, g.steps, g.where.encode() if g.where else b"",
                                [c.expr.encode() for c in g.yields], g.distinct)
        self.device_calls = []
        try:
            k = 0
            while k < len(stages):
                st = stages[k]
                if isinstance(st, GroupBySentence):
                    E = groupby.E
                    nxt = self.b.group_by(rows, names,
                                          [(E.Expr(E.K_FUNC, alias=c.fun, args=[c.expr]) if c.fun else c.expr).encode()
                                           for c in st.groups],
                                          [(c.fun, c.expr.encode(), c.alias) for c in st.yields])
                    names = [c.name() for c in st.yields]
                    self.device_calls.append("group_by")
                    k += 1
                else:
                    factors, limit = [], None
                    if isinstance(st, OrderBySentence):
                        factors = st.factors
                        if k + 1 < len(stages) and isinstance(stages[k + 1], LimitSentence):
                            k += 1
                            limit = (stages[k].offset, stages[k].count)
                    else:
                        limit = (st.offset, st.count)
                    nxt = self.b.order_by(rows, names, factors, limit)
                    self.device_calls.append("order_by")
                    k += 1
                rows.free()
                rows = nxt
            return ngql.Interim(names, rows.fetch())
        finally:
            rows.free()


# ------------------------------------------------------------------------------------ comparing
def key_of(row, cols):
    return tuple(groupby.cell(row[c]) for c in cols)


def rows_counter(rows):
    return Counter(tuple(groupby.cell(v) for v in r) for r in rows)


def check_window(dev_rows, inp: ngql.Interim, factors, limit=None):
    """The device's rows for `ORDER BY factors [| LIMIT limit]` over `inp`, exact where the
    reference is: the rows' factor-key sequence is the model's window of sorted keys; for every key
    value wholly inside the window the device rows of that key are the input's as a multiset; for
    a key value the window's edge cuts they are a sub-multiset of the input's."""
    cols = factor_columns(inp.columns, factors)
    mod = order_model(inp, factors).rows
    lo, hi = window(len(mod), *limit) if limit is not None else (0, len(mod))
    want_keys = [key_of(r, cols) for r in mod[lo:hi]]
    got_keys = [key_of(r, cols) for r in dev_rows]
    assert got_keys == want_keys, "the factor-key sequence differs from the model's window"
    all_n = Counter(key_of(r, cols) for r in inp.rows)
    win_n = Counter(want_keys)
    by_key_inp, by_key_dev = {}, {}
    for r in inp.rows:
        by_key_inp.setdefault(key_of(r, cols), []).append(r)
    for r in dev_rows:
        by_key_dev.setdefault(key_of(r, cols), []).append(r)
    for key, n in win_n.items():
        have, pool = rows_counter(by_key_dev[key]), rows_counter(by_key_inp[key])
        if n == all_n[key]:
            assert have == pool, f"rows of key {key} differ from the input's"
        else:
            assert not (have - pool), f"rows of key {key} are not among the input's"


def tail_factors(query: str):
    """The factors that order a statement's result: those of its last ORDER BY when only LIMITs
    follow it (None otherwise)."""
    sents = [parse_sentence(p) for p in groupby.split_pipes(query)]
    while sents and isinstance(sents[-1], LimitSentence):
        sents.pop()
    return sents[-1].factors if sents and isinstance(sents[-1], OrderBySentence) else None


def same_order(got_rows, exp_rows, cols):
    """Equal as ordered lists up to the order of rows that tie under the factor columns `cols`
    (the reference's std::sort is not stable, so its own order of such rows is an accident)."""
    if len(got_rows) != len(exp_rows):
        return False
    if [key_of(r, cols) for r in got_rows] != [key_of(r, cols) for r in exp_rows]:
        return False
    groups_g, groups_e = {}, {}
    for r in got_rows:
        groups_g.setdefault(key_of(r, cols), []).append(r)
    for r in exp_rows:
        groups_e.setdefault(key_of(r, cols), []).append(r)
    return all(rows_counter(groups_g[k]) == rows_counter(groups_e[k]) for k in groups_e)


def run_case(session: Session, case):
    """(ok, message) for one orderby_golden.json case: status, column names and row count where
    the reference asserts them, and the rows — in order where `ordered` (verifyResult without its
    sort), as a multiset otherwise; `match: false` inverts the row check (ASSERT_FALSE)."""
    st, res = session.status(case["query"])
    if st != case["status"]:
        return False, f"status {st} != {case['status']}"
    if st != "SUCCEEDED":
        return True, "failed as expected"
    if "col_names" in case and res.columns != case["col_names"]:
        return False, f"columns {res.columns} != {case['col_names']}"
    if "row_count" in case and len(res.rows) != case["row_count"]:
        return False, f"{len(res.rows)} rows != {case['row_count']}"
    if "expected" not in case:
        return True, ""
    if case.get("ordered"):
        factors = tail_factors(case["query"])
        cols = factor_columns(res.columns, factors) if factors and res.rows else list(range(len(res.columns)))
        same = same_order(res.rows, case["expected"], cols)
    else:
        same = groupby.multiset(res.rows) == groupby.multiset(case["expected"])
    ok = same == case.get("match", True)
    return ok, "" if ok else f"rows {res.rows} vs {case['expected']} (ordered={case.get('ordered')}, match={case.get('match', True)})"
