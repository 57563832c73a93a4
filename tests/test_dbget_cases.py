"""The batch Db::get's meaning on the CPU: hand-worked cases against the
restatement of tests/dbget_cases.py (dict lookups over the runs, get_cases'
``search`` over the tables, ``b"".join`` for the gather), nrun == 0 against
get_cases' expected results, and the seeded batch the GPU tests use: the
literal loop alone shows a query in every class.  No library call is made."""
import numpy as np

import dbget_cases as D
import get_cases as G
from merge_cases import TOMBSTONE


def batch():
    runs, tabs, keys = D.precedence()
    return D.DbGetBatch([D.Run(runs[0], 3, 5), D.Run(runs[1], 1, 2, one=True)], [G.images(t) for t in tabs], keys,
                        front=3, qfront=1)


def test_precedence_by_hand():
    b = batch()
    res, off, out = b.expected()
    at = {k: i for i, k in reversed(list(enumerate(b.keys)))}
    vals = b.values(res)
    src = lambda k: int(res[at[k]]["table"])  # noqa: E731
    # the same key in run 0, run 1 and table 0: run 0 answers
    assert (src(b"all"), vals[at[b"all"]]) == (0, b"from-run0")
    # a tombstone in run 0 over a value in a table: the tombstone answers
    assert (src(b"dead"), vals[at[b"dead"]], int(res[at[b"dead"]]["val_off"]) >> 63) == (0, TOMBSTONE, 1)
    # a value in run 0 over a tombstone in run 1
    assert (src(b"live"), vals[at[b"live"]], int(res[at[b"live"]]["val_off"]) >> 63) == (0, b"again", 0)
    # an empty value against a miss: res tells them apart, the gather gives neither a byte
    assert (src(b"empty"), vals[at[b"empty"]]) == (0, b"") and src(b"miss") == D.NONE_SOURCE and vals[at[b"miss"]] is None
    assert int(res[at[b"empty"]]["val_off"]) == 0 and int(res[at[b"miss"]]["val_off"]) == 0
    # run 1 only, a run's tombstone, the tables behind the runs
    assert (src(b"old"), vals[at[b"old"]]) == (1, b"run1-only") and (src(b"olddead"), vals[at[b"olddead"]]) == (1, TOMBSTONE)
    assert (src(b"tab"), vals[at[b"tab"]]) == (2, b"table-only") and (src(b"tabdead"), vals[at[b"tabdead"]]) == (2, TOMBSTONE)
    assert src(b"") == D.NONE_SOURCE
    # a duplicate query is gathered twice
    want = [b"from-run0", b"", b"again", b"", b"", b"from-run0", b"run1-only", b"", b"table-only", b"", b"", b""]
    assert out.tobytes() == b"".join(want)
    assert off.tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
    assert res[0] == res[5]
    # and the literal loop agrees
    runs, tabs, keys = D.precedence()
    imgs = [G.images(t) for t in tabs]
    for i, k in enumerate(keys):
        lit = D.literal(b.runs, imgs, k)
        assert (None if lit is None else lit) == (None if vals[i] is None else (int(res[i]["table"]), vals[i])), k


def test_val_off_is_relative_to_the_winning_arena():
    b = batch()
    res, _, _ = b.expected()
    for i, k in enumerate(b.keys):
        s = int(res[i]["table"])
        if s in (0, 1) and int(res[i]["vlen"]):
            off = int(res[i]["val_off"]) & (G.TOMBSTONE_BIT - 1)
            assert b.runs[s].vals.tobytes()[off:off + int(res[i]["vlen"])] == dict(b.runs[s].pairs)[k]


def test_no_runs_equals_get_cases():
    tabs, keys = G.several_tables()
    imgs = [G.images(t) for t in tabs]
    g = G.GetBatch(imgs, keys, front=5, qfront=3)
    res, off, out = D.DbGetBatch([], imgs, keys, front=5, qfront=3).expected()
    assert res.tobytes() == g.expected().tobytes()
    vals = [b"" if v is None or v == TOMBSTONE else v for v in g.values(g.expected())]
    assert out.tobytes() == b"".join(vals) and int(off[-1]) == len(out)


def test_run_sizes_and_queries():
    for m in D.RUN_SIZES:
        pairs = D.run_pairs(m, m)
        assert len(pairs) == m and [k for k, _ in pairs] == sorted(set(k for k, _ in pairs))
        b = D.DbGetBatch([D.Run(pairs, m % 4, m % 3)], [], D.run_queries(pairs))
        res, off, out = b.expected()
        assert int((res["table"] == 0).sum()) == m
        for i, k in enumerate(b.keys):
            assert D.literal(b.runs, [], k) == (None if i >= m else (0, pairs[i][1]))
    lens = set(len(k) for k, _ in D.run_pairs(65, 0))
    assert set(range(18)) | {24, 25} <= lens


def test_the_seeded_batch_has_a_query_in_every_class():
    runs, tabs, keys = D.seeded()
    assert [len(r) for r in runs] == [1000, 1001] and len(tabs) == 8 and len(keys) == 4096
    assert all(250 <= len(t) <= 350 for t in tabs)
    c = D.classes(runs, tabs, keys)
    print("classes", c)
    assert all(v > 0 for v in c.values()) and sum(c.values()) == 4096
    # the dict form of the tables equals the restatement on this batch
    b = D.DbGetBatch([D.Run(r) for r in runs], [G.images(t) for t in tabs], keys[:512])
    slow, fast = b.expected(), b.expected(fast=True, entries=tabs)
    assert all(np.array_equal(x, y) for x, y in zip(slow, fast))
