"""Cases and expected values for the batch Db::get (lsmck_db_get_batch).

The expected values restate the meaning without the library: Db::get_internal
(tokio/db.rs:156-189) asks the memtable, the old memtable and then the tables;
here the memtables are RUNS -- sorted (key, value) pairs -- so a run's get is a
dict lookup (BTreeMap::get, memtable.rs:68-70), the tables' is get_cases'
``search``, and the gathered arena is ``b"".join`` of what Db::get returns
(db.rs:146-151: a Some of the one byte 0 becomes None).
"""
import numpy as np

import get_cases as G
from merge_cases import TOMBSTONE, WAL_CMD_DTYPE, B, POOL

RUN_DTYPE = np.dtype([("keys", "<u8"), ("keys_bytes", "<u8"), ("vals", "<u8"), ("vals_bytes", "<u8"),
                      ("ents", "<u8"), ("nent", "<u8")])
NONE_SOURCE = G.NONE_TABLE


class Run:
    """One run: sorted (key, value) pairs, the keys back to back behind
    ``kfront`` filler bytes in an arena of exactly that size and the values
    behind ``vfront`` bytes in another (``one``: both in one arena, a pair's
    value behind its key), the last key and the last value flush with the
    arenas' ends."""

    def __init__(self, pairs, kfront=0, vfront=0, one=False):
        self.pairs = [(bytes(k), bytes(v)) for k, v in pairs]
        self.ents = np.zeros(len(self.pairs), dtype=WAL_CMD_DTYPE)
        klen = np.array([len(k) for k, _ in self.pairs], dtype=np.uint64)
        vlen = np.array([len(v) for _, v in self.pairs], dtype=np.uint64)
        self.ents["type"], self.ents["klen"], self.ents["vlen"] = 1, klen, vlen
        if one:
            start = kfront + np.cumsum(klen + vlen) - (klen + vlen)
            self.ents["key_off"], self.ents["val_off"] = start, start + klen
            self.keys = np.frombuffer(b"\xCC" * kfront + b"".join(k + v for k, v in self.pairs), dtype=np.uint8)
            self.vals = self.keys
        else:
            self.ents["key_off"] = kfront + np.cumsum(klen) - klen
            self.ents["val_off"] = vfront + np.cumsum(vlen) - vlen
            self.keys = np.frombuffer(b"\xCC" * kfront + b"".join(k for k, _ in self.pairs), dtype=np.uint8)
            self.vals = np.frombuffer(b"\xBB" * vfront + b"".join(v for _, v in self.pairs), dtype=np.uint8)

    def arrays(self):
        return self.keys, self.vals, self.ents

    def lookup(self):
        """{key: (val_off in vals, value)}; an empty value's offset is reported as 0."""
        return {k: (int(o) if v else 0, v) for (k, v), o in zip(self.pairs, self.ents["val_off"].tolist())}


class DbGetBatch:
    """Runs (``Run``) in front of get_cases' tables: ``tables`` and the query
    arena as in ``GetBatch`` (front / qfront: the arenas' residues)."""

    def __init__(self, runs, tables, keys, front=0, qfront=0):
        self.runs = list(runs)
        self.t = G.GetBatch(tables, keys, front=front, qfront=qfront)
        self.keys = self.t.keys
        self.data, self.index, self.spans, self.qkeys, self.q = self.t.data, self.t.index, self.t.spans, self.t.qkeys, self.t.q

    def expected(self, fast=False, entries=None):
        """(res, out_off, out): the results with ``table`` the source number,
        the exclusive scan of the answered lengths and the gathered values."""
        nrun = len(self.runs)
        res = self.t.expected(fast=fast, entries=entries)
        hit = res["table"] != G.NONE_TABLE
        res["table"][hit] += nrun
        looks = [r.lookup() for r in self.runs]
        for i, key in enumerate(self.keys):
            for r, d in enumerate(looks):
                if key in d:
                    off, v = d[key]
                    res[i] = (off | G.TOMBSTONE_BIT if v == TOMBSTONE else off, len(v), r)
                    break
        vals = self.values(res)
        answered = [b"" if v is None or v == TOMBSTONE else v for v in vals]
        off = np.zeros(len(self.keys) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(v) for v in answered])
        return res, off, np.frombuffer(b"".join(answered), dtype=np.uint8)

    def values(self, res):
        """Per query None or the value's bytes (a tombstone: the byte 0) from a result array."""
        arenas = [r.vals.tobytes() for r in self.runs]
        data, out = self.data.tobytes(), []
        for r in res:
            s = int(r["table"])
            if s == NONE_SOURCE:
                out.append(None)
            else:
                a = arenas[s] if s < len(arenas) else data
                off = int(r["val_off"]) & (G.TOMBSTONE_BIT - 1)
                out.append(a[off:off + int(r["vlen"])])
        return out


def literal(runs, tables, key):
    """Db::get_internal, literally: (source, value) or None."""
    for r, run in enumerate(runs):
        d = dict(run.pairs)
        if key in d:
            return r, d[key]
    hit = G.search(tables, key)
    return None if hit is None else (len(runs) + hit[0], hit[2])


# --- cases ------------------------------------------------------------------------------
def precedence():
    """(runs' pairs, tables' entries, queries): the same key in run 0, run 1
    and table 0; a tombstone in run 0 over a value in a table; a value in run 0
    over a tombstone in run 1; an empty value; a miss; a duplicate query."""
    r0 = [(b"all", b"from-run0"), (b"dead", TOMBSTONE), (b"empty", b""), (b"live", b"again")]
    r1 = [(b"all", b"from-run1"), (b"live", TOMBSTONE), (b"old", b"run1-only"), (b"olddead", TOMBSTONE)]
    t0 = [(b"all", b"from-table0"), (b"dead", b"alive-in-table"), (b"tab", b"table-only"), (b"tabdead", TOMBSTONE)]
    t1 = [(b"old", b"shadowed"), (b"tab", b"older"), (b"tabdead", b"older-live")]
    keys = [b"all", b"dead", b"live", b"empty", b"miss", b"all", b"old", b"olddead", b"tab", b"tabdead", b"", b"miss"]
    return [r0, r1], [t0, t1], keys


RUN_SIZES = [0, 1, 2, 63, 64, 65]


def run_pairs(m, seed=0):
    """m pairs with strictly increasing keys of lengths 0..17, 24 and 25, keys
    equal in their first 8 bytes that differ later, proper prefixes."""
    special = sorted(set(POOL + [B[:n] for n in range(18)] + [B[:24], B[:24] + b"!", B[:8] + b"tie-a", B[:8] + b"tie-b",
                                                               B[:8] + b"tie-a\x00"]))
    seed %= len(special)
    numbered = [b"r%04d" % i + b"y" * (i % 19) for i in range(m)]
    keys = sorted((special[seed:] + special[:seed] + numbered)[:m])
    vals = [TOMBSTONE, b"", b"\x00\x00", b"v"]
    return [(k, vals[i % 4] if i % 5 == 0 else b"run%d-%d" % (seed, i) + b"w" * (i % 21)) for i, k in enumerate(keys)]


def run_queries(pairs):
    """Every key of the pairs; below the first, above the last, between two
    keys, a prefix of a key, a key plus one byte, the empty key."""
    return G.queries_for(pairs)


GATHER_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 32767, 32768, 32769, 65537]


def value_of(n, tag):
    """n bytes no two neighbours of which repeat with the period of a chunk."""
    return bytes((tag * 37 + j * 7 + j // 251) % 253 + 1 for j in range(n))


def seeded(seed=5, nrun=(1000, 1000), ntab=8, nq=4096):
    """2 runs of about 1,000 entries, 8 tables of about 300 and 4,096 queries:
    (runs' pairs, tables' entries, query keys).  Keys are numbers drawn from
    one range, so a key lies in a run, in a table, in both or nowhere; a value
    is a tombstone where the number says so."""
    rng = np.random.default_rng(seed)

    def ents(m, tag):
        nums = np.sort(rng.choice(6000, size=m, replace=False)).tolist()
        out = [(b"key%08d" % x + b"s" * (x % 5), TOMBSTONE if (x + tag) % 11 == 0 else b"%c%d-" % (tag + 65, x) + b"v" * (x % 29))
               for x in nums]
        return sorted(out)
    runs = [ents(m + r, r) for r, m in enumerate(nrun)]
    tables = [ents(int(rng.integers(250, 351)), 2 + t) for t in range(ntab)]
    keys = []
    for i in range(nq):
        x = int(rng.integers(0, 6500))
        keys.append(b"key%08d" % x + b"s" * ((x + (i % 7 == 0)) % 5))
    return runs, tables, keys


def classes(runs, tables, keys):
    """How many queries fall in each class, from the literal loop alone."""
    imgs = [G.images(t) for t in tables]
    maps = [G.btreemap(x) for _, x in imgs]
    out = dict(run0=0, run1_only=0, table=0, run_tombstone=0, table_tombstone=0, miss=0)
    seen = {}
    for k in keys:
        if k not in seen:
            hit = None
            for r, pairs in enumerate(runs):
                d = dict(pairs)
                if k in d:
                    hit = (r, d[k])
                    break
            if hit is None:
                s = G.search(imgs, k, maps)
                hit = None if s is None else (len(runs) + s[0], s[2])
            seen[k] = hit
        hit = seen[k]
        if hit is None:
            out["miss"] += 1
        elif hit[1] == TOMBSTONE:
            out["run_tombstone" if hit[0] < len(runs) else "table_tombstone"] += 1
        elif hit[0] == 0:
            out["run0"] += 1
        elif hit[0] == 1 and len(runs) > 1:
            out["run1_only"] += 1
        else:
            out["table"] += 1
    return out
