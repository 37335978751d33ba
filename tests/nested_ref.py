"""A plain-Python restatement of the reference's filter evaluation, Nested nodes included (query/filters.rs:13-188 over
index/fastfields.rs:802-907), over per-doc / per-object value lists.  It compares strings and integers and shares no
code with searchlite_amd: it is what the device's bitmaps are compared with.

A world is one segment:
    {"n_docs": n,
     "kinds":   {column name: "keyword" | "i64" | "f64"}     doc-level columns and nested ones ("path.field")
     "doc":     {field: [values of doc 0, values of doc 1, ...]}
     "counts":  {path: [objects of doc 0, ...]}               _nested_count:<path> (may be shorter than n_docs)
     "parents": {path: [[parent index or None per object] per doc]}   _nested_parent:<path> (absent: no column)
     "nested":  {"path.field": [[[values of object 0], [values of object 1], ...] per doc]}}
A nested column may hold fewer objects for a doc than the path counts, and fewer docs than the segment.
"""


def case_insensitive_equals(a, b):
    """index/fastfields.rs:475-481"""
    if a.isascii() and b.isascii():
        return len(a) == len(b) and all(x.lower() == y.lower() for x, y in zip(a, b))
    return a.lower() == b.lower()


def _qualified(base, field):
    return field if not base else base + "." + field


def _object_count(world, path, doc):
    counts = world.get("counts", {}).get(path)
    return counts[doc] if counts is not None and doc < len(counts) else 0


def _parents(world, path, doc):
    col = world.get("parents", {}).get(path)
    return col[doc] if col is not None and doc < len(col) else []


def _values(world, name, kind, doc, idx):
    """the values a leaf of `kind` sees: of the doc (idx None) or of its object idx; a column of another kind, or
    none, gives nothing, and so does an object the column does not reach"""
    if world.get("kinds", {}).get(name) != kind:
        return []
    if idx is None:
        col = world.get("doc", {}).get(name)
        return col[doc] if col is not None and doc < len(col) else []
    col = world.get("nested", {}).get(name)
    objects = col[doc] if col is not None and doc < len(col) else []
    return objects[idx] if idx < len(objects) else []


def filter_matches(world, doc, flt, base="", idx=None):
    (tag, body), = flt.items()
    if tag == "KeywordEq":
        vals = _values(world, _qualified(base, body["field"]), "keyword", doc, idx)
        return any(case_insensitive_equals(v, body["value"]) for v in vals)
    if tag == "KeywordIn":
        vals = _values(world, _qualified(base, body["field"]), "keyword", doc, idx)
        return any(case_insensitive_equals(t, v) for v in vals for t in body["values"])
    if tag == "I64Range":
        vals = _values(world, _qualified(base, body["field"]), "i64", doc, idx)
        return any(body["min"] <= v <= body["max"] for v in vals)
    if tag == "F64Range":
        vals = _values(world, _qualified(base, body["field"]), "f64", doc, idx)
        return any(v >= body["min"] and v <= body["max"] for v in vals)  # (a NaN on either side: False)
    if tag == "Nested":
        return _nested_passes(world, doc, base, body["path"], idx, [body["filter"]], grouped=False)
    if tag == "And":
        return passes_filters_at(world, doc, body, base, idx)
    if tag == "Or":
        return any(filter_matches(world, doc, child, base, idx) for child in body)
    if tag == "Not":
        return not filter_matches(world, doc, body, base, idx)
    raise ValueError(tag)


def passes_filters_at(world, doc, filters, base="", idx=None):
    """filters.rs:13-50: the Nested children of one list that share a path must hold for ONE object"""
    groups = {}
    for flt in filters:
        if list(flt) == ["Nested"]:
            groups.setdefault(flt["Nested"]["path"], []).append(flt["Nested"]["filter"])
        elif not filter_matches(world, doc, flt, base, idx):
            return False
    return all(_nested_passes(world, doc, base, path, idx, group, grouped=True) for path, group in groups.items())


def _nested_passes(world, doc, base, path, parent_idx, filters, grouped):
    """nested_group_passes (grouped) / nested_filter_passes: some object of base.path, bound to parent_idx when
    there is one, passes"""
    full = _qualified(base, path)
    parents = _parents(world, full, doc)
    for i in range(_object_count(world, full, doc)):
        if parent_idx is not None and (i >= len(parents) or parents[i] is None or parents[i] != parent_idx):
            continue
        if grouped:
            if passes_filters_at(world, doc, filters, full, i):
                return True
        elif filter_matches(world, doc, filters[0], full, i):
            return True
    return False


def mask(world, flt):
    """the docs of the segment that pass flt (passes_filter), as a list of booleans"""
    return [filter_matches(world, d, flt) for d in range(world["n_docs"])]
