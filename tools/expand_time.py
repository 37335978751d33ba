"""Time of term expansion (slg_expand_batch) at config 2's scale: a Zipf-like vocabulary of 2^18 words generated
here (word of rank r = term id r of the 1M-doc Zipf segment), one segment, and a batch of 1024 three-term queries
under the default FuzzyOptions (1 edit, prefix 1, 50 expansions, min length 3), then the same with prefix_length 0.
Per batch, mean of `reps` calls after two warm-up calls, `rounds` times over so the spread shows:
  * slg_expand_batch: the whole call by the host clock (the call ends in a stream synchronise), and its own split
    into the device scan (uploads, both kernels, the copy back, the wait) and the host merge (slg_expand_phase_ms);
  * the same expansions by the C++ restatement of the reference's loop (csrc/slg_expand_capi.cpp,
    slgx_reference_expand: what a caller without the scan runs) on this box, at 1 and 16 threads; the 1-thread
    prefix-0 figure is timed on every 8th request and multiplied by 8 (stated in the line);
  * for context the plain scoring batch that follows (the source terms as a plain batch, k = 11): HIP events around
    slg_batch_run, and search_fuzzy (8 expansions per term, so that every query stays under the scoring kernels' 32-term
    cap) end to end through the Python layer, whose folding loop is most of that figure.
The device's answer is compared with the restatement's before anything is timed.

Regex mode (`regex` as the first argument): on the same vocabulary, 1024 wildcard requests `ab*c?` (the first two
letters of a word, any run, one of its later letters, one char; 50 expansions) and the same patterns written as
regexes, `ab.*c.`: the same ranges and the same answers, which is asserted before anything is timed; then one pattern
with an empty literal prefix, `.*ing` beside the wildcard `*ing`, whose range is the whole field.  Per batch the
whole call, the device scan and the host merge as above.  `wildcard` as the first argument times the wildcard
batches alone: the yardstick, for a library built from a commit without the regex kind (SLG_LIB_TAG).
usage (GPU box): python tools/expand_time.py [regex | wildcard] [reps] [rounds]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from searchlite_amd import build, corpus, searcher, _native as N  # noqa: E402
from tools.vocabulary import make_vocabulary  # noqa: E402

mode = sys.argv.pop(1) if len(sys.argv) > 1 and sys.argv[1] in ("regex", "wildcard") else "fuzzy"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n_docs, vocab, nq, T = 1_000_000, 1 << 18, 1024, 3


t0 = time.time()
words = make_vocabulary(vocab)
keys = ["body:" + w for w in words]
seg = corpus.zipf_segment(n_docs, vocab, seed=42, n_threads=16)
offs, terms, w = corpus.zipf_queries(nq, T, seed=7, vocab=vocab)
ix = searcher.GpuIndex([seg])
ix.set_stream(torch.cuda.current_stream().cuda_stream)
ix.set_terms(0, keys)
lens = np.array([len(x) for x in words])
first = np.array([x[0] for x in words])
print(json.dumps(dict(vocabulary=len(words), mean_chars=round(float(lens.mean()), 2), segments=1, docs=n_docs,
                      queries=nq, terms_per_query=T,
                      largest_prefix1_range=int(max((first == c).sum() for c in set(first.tolist()))),
                      setup_s=round(time.time() - t0, 1))), flush=True)

# the host restatement over the library's own host dictionary
L = C.CDLL(build.build_plan_lib())
L.slgx_dict_build.restype = C.c_void_p
L.slgx_dict_build.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p]
L.slgx_reference_expand.restype = C.c_int
L.slgx_reference_expand.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
raw = [k.encode() for k in keys]
koffs = np.zeros(len(raw) + 1, dtype=np.uint32)
np.cumsum([len(r) for r in raw], out=koffs[1:])
blob = np.frombuffer(b"".join(raw), dtype=np.uint8)
err = C.create_string_buffer(256)
hd = L.slgx_dict_build(len(raw), blob.ctypes.data, koffs.ctypes.data, err, 256, None)
assert hd, err.value
dicts = (C.c_void_p * 1)(hd)


def c_reqs(reqs):
    keep = []
    arr = (N.ExpandReq * len(reqs))()
    for i, r in enumerate(reqs):
        f, t = r["field"].encode(), r["term"].encode()
        keep += [f, t]
        arr[i] = N.ExpandReq(C.sizeof(N.ExpandReq), r["kind"], f, t, len(f), len(t), r["max_expansions"], r["max_edits"],
                             r["prefix_length"], r["min_length"])
    return arr, keep


def host_loop(reqs, n_threads, want_rows=False):
    arr, keep = c_reqs(reqs)
    o = np.zeros(len(reqs) + 1, dtype=np.uint32)
    cap = len(reqs) * 51
    ids = np.zeros((cap, 1), np.uint32) if want_rows else None
    dist = np.zeros(cap, np.uint8) if want_rows else None
    t = time.perf_counter()
    rc = L.slgx_reference_expand(dicts, 1, arr, len(reqs), n_threads, o.ctypes.data, cap,
                                 None if ids is None else ids.ctypes.data, None if dist is None else dist.ctypes.data, err, 256)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, err.value
    return ms, o, ids, dist


def scoring_context():
    b = ix.prepare(offs, terms, w, 11, searcher.Wand)
    try:
        for _ in range(2):
            b.run()
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            b.run()
        e.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(e) / 10, 4)
    finally:
        b.close()


def time_batch(label, reqs):
    """`rounds` lines for one batch: the call, its scan and its merge, mean of `reps` after two warm-up calls"""
    arr, keep = c_reqs(reqs)
    cap = max(sum(r["max_expansions"] for r in reqs), 1)
    o, out_ids, out_dist = np.zeros(len(reqs) + 1, np.uint32), np.zeros((cap, 1), np.uint32), np.zeros(cap, np.uint8)

    def one_call():
        N.check(ix._lib.slg_expand_batch(ix._h, arr, len(reqs), o.ctypes.data, cap, out_ids.ctypes.data, out_dist.ctypes.data))
    one_call()
    one_call()
    for rnd in range(rounds):
        call, scan, merge = [], [], []
        for _ in range(reps):
            t = time.perf_counter()
            one_call()
            call.append((time.perf_counter() - t) * 1e3)
            sc, mg = ix.expand_phase_ms()
            scan.append(sc)
            merge.append(mg)
        print(json.dumps(dict(round=rnd, batch=label, requests=len(reqs), keys=int(o[-1]),
                              expand_call_ms=round(float(np.mean(call)), 3), device_scan_ms=round(float(np.mean(scan)), 3),
                              host_merge_ms=round(float(np.mean(merge)), 3))), flush=True)


if mode != "fuzzy":
    rng = np.random.default_rng(11)
    long_words = [x for x in words if len(x) >= 5]
    pairs = []
    for i in rng.choice(len(long_words), size=nq, replace=False):
        x = long_words[int(i)]
        pairs.append((x[:2] + "*" + x[3] + "?", x[:2] + ".*" + x[3] + "."))
    wild = [searcher.expand_request(N.EXPAND_WILDCARD, "body", a, 50) for a, _ in pairs]
    wild_all = [searcher.expand_request(N.EXPAND_WILDCARD, "body", "*ing", 50)]
    if mode == "regex":
        rx = [searcher.expand_request(N.EXPAND_REGEX, "body", b, 50) for _, b in pairs]
        rx_all = [searcher.expand_request(N.EXPAND_REGEX, "body", ".*ing", 50)]
        for a, b in ((wild, rx), (wild_all, rx_all)):           # the same answers before any timing
            for i, ((ia, da), (ib, db)) in enumerate(zip(ix.expand(a), ix.expand(b))):
                assert ia.tolist() == ib.tolist() and da.tolist() == db.tolist(), (i, a[i], b[i])
        host = host_loop(rx, 16)[1]                             # and the C++ restatement of the loop counts as many
        assert int(host[-1]) == sum(len(d) for _, d in ix.expand(rx))
    first2 = np.array([x[:2] for x in words])
    print(json.dumps(dict(mode=mode, library=os.path.basename(N.lib_path()), patterns="ab*c? / ab.*c.",
                          mean_range_keys=round(float(np.mean([(first2 == a[:2]).sum() for a, _ in pairs])), 1),
                          whole_field_keys=len(words))), flush=True)
    time_batch("wildcard ab*c?", wild)
    if mode == "regex":
        time_batch("regex ab.*c.", rx)
    time_batch("wildcard *ing (empty literal prefix)", wild_all)
    if mode == "regex":
        time_batch("regex .*ing (empty literal prefix)", rx_all)
        t = time.perf_counter()
        host_loop(rx, 16)
        cpu16 = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        host_loop(rx_all, 1)
        print(json.dumps(dict(cpu_dfa_loop_16_threads_ms_ab=round(cpu16, 1),
                              cpu_dfa_loop_1_thread_ms_ing=round((time.perf_counter() - t) * 1e3, 1),
                              note="slgx_reference_expand with the host build of the DFA walk, not the reference's regex engine")), flush=True)
    sys.exit(0)

for prefix_length in (1, 0):
    fz = dict(max_edits=1, prefix_length=prefix_length, max_expansions=50, min_length=3)
    reqs = [searcher.expand_request(N.EXPAND_FUZZY, "body", words[int(t)], **fz) for t in terms.reshape(-1)]
    arr, keep = c_reqs(reqs)
    o, out_ids, out_dist = np.zeros(len(reqs) + 1, np.uint32), np.zeros((len(reqs) * 51, 1), np.uint32), np.zeros(len(reqs) * 51, np.uint8)

    def one_call():
        N.check(ix._lib.slg_expand_batch(ix._h, arr, len(reqs), o.ctypes.data, len(out_dist), out_ids.ctypes.data,
                                         out_dist.ctypes.data))
    got = ix.expand(reqs)                                   # (also the first warm-up call)
    _, ro, rids, rdist = host_loop(reqs, 16, want_rows=True)
    for i, (ids, dist) in enumerate(got):                   # the same answer before any timing
        assert ids[:, 0].tolist() == rids[ro[i]:ro[i + 1], 0].tolist() and dist.tolist() == rdist[ro[i]:ro[i + 1]].tolist(), i
    n_keys = int(ro[-1])
    one_call()
    assert o.tolist() == ro.tolist()
    for rnd in range(rounds):
        call, scan, merge = [], [], []
        for _ in range(reps):
            t = time.perf_counter()
            one_call()
            call.append((time.perf_counter() - t) * 1e3)
            s, m = ix.expand_phase_ms()
            scan.append(s)
            merge.append(m)
        sub = reqs[::8] if prefix_length == 0 else reqs
        cpu1 = host_loop(sub, 1)[0] * (len(reqs) / len(sub))
        cpu16 = host_loop(reqs, 16)[0]
        print(json.dumps(dict(round=rnd, prefix_length=prefix_length, requests=len(reqs), keys=n_keys,
                              expand_call_ms=round(float(np.mean(call)), 3),
                              device_scan_ms=round(float(np.mean(scan)), 3), host_merge_ms=round(float(np.mean(merge)), 3),
                              cpu_loop_1_thread_ms=round(cpu1, 1), cpu_1_thread_timed_on="every 8th request, x8" if len(sub) != len(reqs) else "all requests",
                              cpu_loop_16_threads_ms=round(cpu16, 1))), flush=True)

plain_ms = scoring_context()
queries = [" ".join(words[int(t)] for t in terms.reshape(-1)[q * T:(q + 1) * T]) for q in range(nq)]
fz8 = dict(max_edits=1, prefix_length=1, max_expansions=8, min_length=3)   # (3 x 9 keys stay under the 32-term cap)
ix.search_fuzzy(queries[:64], "body", 11, fz8)
t = time.perf_counter()
ix.search_fuzzy(queries, "body", 11, fz8)
fuzzy_ms = round((time.perf_counter() - t) * 1e3, 1)
print(json.dumps(dict(plain_scoring_batch_ms=plain_ms, search_fuzzy_8_expansions_python_host_ms=fuzzy_ms)), flush=True)
