"""The world of tests/test_gpu_nested_filters.py, built on the CPU: per segment a tests/nested_ref.py world (the
reference's view), the arrays it registers as (the fast-field file's view), the families of filters, and an
interpreter of compile_nested_filter's programs over the reference's view.  tests/test_nested_ref.py checks on the
CPU that the world has the edges the kernel can go wrong at and that every family passes some live docs and fails
some: a family whose reference mask is all-true or all-false everywhere would hide a broken kernel.

Paths: c (comments), c.r (replies, bound to comments), c.r.z (a third level), e (a path that is empty in one segment
and has no count column in another).  Docs hold 0, 1, 2 or 5 comments; one doc per segment of 64 docs and up holds 70,
and the count of the doc before it is chosen so that its object range starts at bit 32, 31 or 63 of a wave's 64
bits."""
import numpy as np

SIZES = (1, 33, 64, 65, 257)
SEED = 20261020
BIG = 70
BIG_START = {64: 32, 65: 31, 257: 63}    # segment size -> (first object of the 70-object doc) % 64
I64_MIN, I64_MAX, TWO53 = -2**63, 2**63 - 1, 2**53
INF, NAN = float("inf"), float("nan")
AUTHORS = [f"a{o}" for o in range(33)]
AUTHORS[1] = "A0"                        # equal to a0 under case_insensitive_equals: two ordinals for one value
TAGS = ["x", "y", "z", "Y", "w"]
CATS = ["news", "blog", "wiki"]
STARS = [I64_MIN, I64_MIN + 1, -TWO53 - 1, -3, 0, 3, 7, TWO53, TWO53 + 1, I64_MAX - 1, I64_MAX]
SCORES = [NAN, INF, -INF, -0.0, 0.0, 0.5, 1.5, -1.5, 2.5]
KINDS = {"cat": "keyword", "n": "i64", "c.author": "keyword", "c.score": "f64", "c.stars": "i64", "c.r.tag": "keyword",
         "c.r.n": "i64", "c.r.z.v": "f64", "e.k": "i64"}
PATH_PARENT = {"c": None, "c.r": "c", "c.r.z": "c.r", "e": None}
MAX = 0xFFFFFFFF


def _segment(rng, n, s):
    """one segment's nested_ref world"""
    c = [(0, 1, 2, 5)[d % 4] for d in range(n)]
    if n == 1:
        c = [2]
    if n in BIG_START:
        big = n // 2
        before = sum(c[:big - 1])
        c[big - 1] = (BIG_START[n] - before) % 64
        c[big] = BIG
    r = [(2, 0, 5, 1)[d % 4] for d in range(n)]
    z = [(1, 2, 0)[d % 3] for d in range(n)]
    e = [int(rng.integers(0, 3)) for _ in range(n)]
    w = {"n_docs": n, "kinds": dict(KINDS), "doc": {}, "counts": {"c": c, "c.r": r, "c.r.z": z, "e": e}, "parents": {},
         "nested": {}}
    if s == 1:
        w["counts"]["e"] = [0] * n        # a segment whose path has no object at all
    if s == 2:
        del w["counts"]["e"]              # a segment registered with NULL counts

    def parents(count, above, p_none=0.15, p_out=0.1):
        out = []
        for d in range(n):
            row = []
            for _ in range(count[d]):
                u = rng.random()
                if u < p_none:
                    row.append(None)                     # u32::MAX
                elif u < p_none + p_out or above[d] == 0:
                    row.append(above[d] + int(rng.integers(0, 3)))   # out of range
                else:
                    row.append(int(rng.integers(0, above[d])))
            if d % 7 == 3 and row:
                row = row[:-1]                            # a list shorter than the count
            out.append(row)
        return out

    if s != 3:                                            # (segment 3: no parent column for c.r: nothing binds)
        w["parents"]["c.r"] = parents(r, c)
    w["parents"]["c.r.z"] = parents(z, r, p_none=0.05, p_out=0.05)
    w["parents"]["c"] = [[None] * k for k in c]           # top-level objects carry u32::MAX (read by nobody)

    def column(count, draw, sizes=(0, 1, 3), trim=True):
        out = []
        for d in range(n):
            objs = [[draw() for _ in range(sizes[int(rng.integers(0, len(sizes)))])] for _ in range(count[d])]
            while trim and objs and not objs[-1]:
                objs.pop()                                # padded only up to the last object that had a value
            out.append(objs)
        return out

    pick = lambda a: (lambda: a[int(rng.integers(0, len(a)))])
    w["nested"]["c.author"] = column(c, pick(AUTHORS[:8] + [AUTHORS[32]]))
    w["nested"]["c.score"] = column(c, pick(SCORES))
    w["nested"]["c.stars"] = column(c, pick(STARS))
    w["nested"]["c.r.tag"] = column(r, pick(TAGS))
    w["nested"]["c.r.n"] = column(r, lambda: int(rng.integers(-2, 3)))
    w["nested"]["c.r.z.v"] = column(z, lambda: float(rng.integers(-4, 5)) / 2.0, sizes=(0, 1, 1, 3))
    if "e" in w["counts"]:
        w["nested"]["e.k"] = column(w["counts"]["e"], lambda: int(rng.integers(0, 4)))
    if s == 4:
        del w["nested"]["c.r.n"]                          # a value column registered with NULL for this segment
    w["doc"]["cat"] = [[CATS[int(rng.integers(0, 3))]] if d % 5 else [] for d in range(n)]
    w["doc"]["n"] = [[int(rng.integers(-5, 6))] for _ in range(n)]
    dead = rng.random(n) < (0.15 if n > 1 else 0.0)
    if n in (33, 65, 257):
        dead[-1] = True
    return w, dead


def build(sizes=SIZES, seed=SEED):
    """-> (worlds, dead): one nested_ref world and one tombstone mask per segment"""
    rng = np.random.default_rng(seed)
    made = [_segment(rng, n, s) for s, n in enumerate(sizes)]
    return [m[0] for m in made], [m[1] for m in made]


# ---- the reference's view as the arrays the fast-field file holds --------------------------------------------
def path_arrays(w, path):
    """-> None (no count column), or (counts u32[n_docs], (parent offsets, parents) or None)"""
    if path not in w["counts"]:
        return None
    counts = np.asarray(w["counts"][path], np.uint32)
    if path not in w["parents"]:
        return counts
    rows = w["parents"][path]
    offs = np.zeros(w["n_docs"] + 1, np.uint32)
    offs[1:] = np.cumsum([len(r) for r in rows])
    vals = np.asarray([MAX if p is None else p for r in rows for p in r], np.uint32)
    return counts, (offs, vals)


def column_arrays(w, name, keys=None):
    """-> None (no column in this segment), or (doc offsets, object offsets, values)"""
    if name not in w["nested"]:
        return None
    docs = w["nested"][name]
    doc_offs = np.zeros(w["n_docs"] + 1, np.uint32)
    doc_offs[1:] = np.cumsum([len(o) for o in docs])
    objs = [v for o in docs for v in o]
    obj_offs = np.zeros(len(objs) + 1, np.uint32)
    obj_offs[1:] = np.cumsum([len(v) for v in objs])
    flat = [x for v in objs for x in v]
    kind = w["kinds"][name]
    if kind == "keyword":
        vals = np.asarray([keys.index(x) for x in flat], np.uint32)
    else:
        vals = np.asarray(flat, np.int64 if kind == "i64" else np.float64)
    return doc_offs, obj_offs, vals


KEYS = {"c.author": AUTHORS, "c.r.tag": TAGS, "cat": CATS}


# ---- the families of filters -------------------------------------------------------------------------------
keq = lambda f, v: {"KeywordEq": {"field": f, "value": v}}
kin = lambda f, vs: {"KeywordIn": {"field": f, "values": vs}}
i64 = lambda f, lo, hi: {"I64Range": {"field": f, "min": lo, "max": hi}}
f64 = lambda f, lo, hi: {"F64Range": {"field": f, "min": lo, "max": hi}}
nest = lambda p, f: {"Nested": {"path": p, "filter": f}}
AND = lambda *f: {"And": list(f)}
OR = lambda *f: {"Or": list(f)}
NOT = lambda f: {"Not": f}

FAMILIES = {
    "lone keyword": [nest("c", keq("author", "a0")), nest("c", kin("author", ["A2", "a32", "nobody"]))],
    "one path twice in And and in Or": [
        AND(nest("c", keq("author", "a0")), nest("c", f64("score", 0.5, 2.5))),
        OR(nest("c", keq("author", "a0")), nest("c", f64("score", 0.5, 2.5))),
        AND(nest("c", keq("author", "a3")), nest("c", i64("stars", -3, 7)), keq("cat", "NEWS"))],
    "under Not": [NOT(nest("c", keq("author", "a0"))), NOT(nest("e", i64("k", 0, 1))),
                  AND(NOT(nest("c", f64("score", -INF, INF))), i64("n", -5, 3))],
    "f64 edges": [nest("c", f64("score", -INF, INF)), nest("c", f64("score", INF, INF)),
                  nest("c", f64("score", -0.0, 0.0)), nest("c", AND(f64("score", 1.5, 1.5), NOT(f64("score", -INF, 0.5))))],
    "i64 edges": [nest("c", i64("stars", I64_MIN, I64_MIN)), nest("c", i64("stars", I64_MAX, I64_MAX)),
                  nest("c", i64("stars", TWO53 + 1, TWO53 + 1)), nest("c", i64("stars", TWO53, TWO53)),
                  nest("c", i64("stars", -TWO53 - 1, -4)), nest("c", i64("stars", I64_MIN + 1, I64_MAX - 1))],
    "two levels": [nest("c", AND(keq("author", "a0"), nest("r", keq("tag", "y")))),
                   nest("c", nest("r", i64("n", 1, 2))),
                   nest("c", OR(nest("r", keq("tag", "x")), nest("r", keq("tag", "w")))),
                   nest("c", AND(nest("r", keq("tag", "x")), nest("r", i64("n", -2, 0)), f64("score", -INF, INF)))],
    "three levels": [nest("c", nest("r", nest("z", f64("v", 0.5, 2.0)))),
                     nest("c", AND(NOT(keq("author", "a1")), nest("r", AND(keq("tag", "y"), nest("z", f64("v", -2.0, 0.0))))))],
    "dotted path at the doc level": [nest("c.r", keq("tag", "y")), nest("c.r.z", f64("v", 1.0, 2.0)),
                                     AND(nest("c.r", keq("tag", "x")), nest("c.r", i64("n", 0, 2)))],
    "empty and missing paths": [nest("e", i64("k", 0, 1)), OR(nest("e", i64("k", 2, 3)), keq("cat", "wiki"))],
    "unknown names and wrong kinds": [
        OR(nest("nope", keq("author", "a0")), nest("c", keq("score", "a0")), nest("c", i64("score", 0, 9)),
           nest("c", keq("cat", "news")), nest("c", keq("author", "a0"))),
        AND(NOT(nest("c", nest("z", f64("v", -9.0, 9.0)))), NOT(nest("c", f64("stars", -INF, INF))), keq("cat", "news")),
        OR(nest("c", nest("nope", keq("tag", "x"))), nest("c", f64("score", NAN, 1.0)), i64("n", 0, 5))],
}


# ---- an interpreter of compile_nested_filter's programs over the reference's view ----------------------------
def describe(path_ids, field_ids):
    """the `nested` argument of compile_nested_filter and the doc-level `fields`, from name -> id maps"""
    nested = {"paths": {p: {"id": i} for p, i in path_ids.items()}, "fields": {}}
    fields = {}
    for name, fid in field_ids.items():
        d = {"id": fid, "kind": KINDS[name], "keys": KEYS.get(name)}
        if "." in name:
            d["path"] = name.rsplit(".", 1)[0]
            nested["fields"][name] = d
        else:
            fields[name] = d
    return fields, nested


def run_program(prog, w, path_ids, field_ids):
    """the docs of segment world w that pass the program (scopes, nodes, ords) -> list of booleans"""
    path_name = {i: p for p, i in path_ids.items()}
    field_name = {(("." in n), i): n for n, i in field_ids.items()}
    KW, F64, I64, FID, AND_, OR_, NOT_, NESTED = range(8)

    def values(name, doc, idx):
        if idx is None:
            col = w["doc"].get(name)
            return col[doc] if col is not None else []
        col = w["nested"].get(name)
        objs = col[doc] if col is not None else []
        return objs[idx] if idx < len(objs) else []

    def scope(si, doc, idx):
        path, begin, count = prog.scopes[si]
        stack = []
        for nd in prog.nodes[begin:begin + count]:
            k = nd["kind"]
            if k in (KW, F64, I64):
                name = field_name[(idx is not None, nd["field"])]
                vals = values(name, doc, idx)
                if k == KW:
                    ords = set(prog.ords[nd["ord_begin"]:nd["ord_begin"] + nd["n_ords_in"]])
                    stack.append(any(KEYS[name].index(v) in ords for v in vals))
                elif k == F64:
                    stack.append(any(nd["lo_f"] <= v <= nd["hi_f"] for v in vals))
                else:
                    stack.append(any(nd["lo_i"] <= v <= nd["hi_i"] for v in vals))
            elif k == NESTED:
                child = path_name[prog.scopes[nd["field"]][0]]
                counts = w["counts"].get(child)
                par = w["parents"].get(child)
                rows = par[doc] if par is not None else []
                hit = False
                for j in range(counts[doc] if counts is not None else 0):
                    if idx is not None and (j >= len(rows) or rows[j] is None or rows[j] != idx):
                        continue
                    if scope(nd["field"], doc, j):
                        hit = True
                        break
                stack.append(hit)
            elif k == NOT_:
                stack.append(not stack.pop())
            elif k in (AND_, OR_):
                top = [stack.pop() for _ in range(nd["arity"])]
                stack.append(all(top) if k == AND_ else any(top))
            else:
                raise AssertionError(f"kind {k} in a compiled nested program")
        assert len(stack) == 1
        return stack[0]

    return [scope(len(prog.scopes) - 1, d, None) for d in range(w["n_docs"])]
