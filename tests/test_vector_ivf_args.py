"""slg_index_cluster_vector_field / slg_index_fetch_vector_lists / slg_vector_search_batch_ivf[_device]: the exports,
their ctypes signatures against the header and the Rust mirror, the Python wrappers, and the argument errors that need
no device: nprobe and cand_size are checked before the index is looked at, and a NULL index or NULL clause_field fails
with SLG_ERR_INVALID and a message before anything touches a GPU (as tests/test_vector_approx_args.py does for the
two-pass call).  Then searchlite_amd.ivf.train_centroids, which runs on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH = ["slg_vector_search_batch_ivf", "slg_vector_search_batch_ivf_device"]
vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
SIGS = {
    "slg_index_cluster_vector_field": [vp, u32, vp, u32],
    "slg_index_fetch_vector_lists": [vp, u32, u32, vp, vp, vp, u32, u32],
    SEARCH[0]: [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp],
    SEARCH[1]: [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp],
}


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)


def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(SIGS))
def test_exports_and_signatures(lib, name):
    assert hasattr(lib, name), f"{name} is not exported"
    fn = getattr(lib, name)
    assert fn.restype is i32 and list(fn.argtypes) == SIGS[name]
    assert _n_args(_header(), r"\b%s\s*\((.*?)\)\s*;" % name) == len(SIGS[name])
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    assert _n_args(rs, r"pub fn %s\((.*?)\)\s*->" % name) == len(SIGS[name])


def test_limits_in_the_header_the_mirror_and_python():
    from searchlite_amd import _native as N
    header = open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for name, value in (("MAX_VECTOR_LISTS", 65536), ("MAX_VECTOR_PROBES", 256), ("KEEP_VECTOR_LISTS", 0xFFFFFFFF)):
        h = re.search(r"#define\s+SLG_%s\s+(\w+)u\b" % name, header)
        assert h and int(h.group(1), 0) == value
        r = re.search(r"pub const SLG_%s: u32 = ([\w_]+);" % name, rs)
        assert r and int(r.group(1).replace("_", ""), 0) == value
        assert getattr(N, name) == value
    assert re.search(r"struct slg_vector_lists_desc\s*\{\s*pub n_lists: u32,\s*pub centroids: \*const c_float\s*\}", rs)
    assert C.sizeof(N.VectorListsDesc) == 16


def test_nprobe_follows_cand_size_in_the_header():
    header = _header()
    for name in SEARCH:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, header, re.S).group(1)
        names = [a.split()[-1].lstrip("*") for a in args.split(",")]
        assert names[8:11] == ["cand_size", "nprobe", "k_out"]


def test_python_wrappers_exist():
    from searchlite_amd import GpuIndex
    from searchlite_amd import ivf
    for m in ("cluster_vector_field", "fetch_vector_lists", "vector_search_ivf", "vector_search_ivf_device"):
        assert callable(getattr(GpuIndex, m))
    assert callable(ivf.train_centroids)


def _args(cand=5, nprobe=2):
    nq, dim, k = 2, 4, 3
    keep = dict(cf=np.zeros(1, np.uint32), q=np.zeros((nq, dim), np.float32), a=np.zeros((nq, 1), np.float32),
                doc=np.full((nq, k), 7, np.uint32), seg=np.full((nq, k), 7, np.uint32),
                sc=np.full((nq, k), 7, np.float32), vs=np.full((nq, k), 7, np.float32),
                cnt=np.full(nq, 7, np.uint32), tot=np.full(nq, 7, np.uint64))
    p = {n: a.ctypes.data for n, a in keep.items()}
    return keep, [nq, 1, p["cf"], p["q"], p["a"], None, None, cand, nprobe, k, p["doc"], p["seg"], p["sc"], p["vs"],
                  p["cnt"], p["tot"]]


def _untouched(keep):
    return all((keep[n] == 7).all() for n in ("doc", "seg", "sc", "vs", "cnt", "tot"))


@pytest.mark.parametrize("name", SEARCH)
@pytest.mark.parametrize("cand,nprobe,word", [(5, 0, b"nprobe"), (5, 257, b"nprobe"), (5, 0xFFFFFFFF, b"nprobe"),
                                              (65, 0, b"nprobe"), (65, 1, b"cand_size"), (10000, 256, b"cand_size")])
def test_nprobe_and_cand_size_outside_their_range_are_unsupported(lib, name, cand, nprobe, word):
    """nprobe outside 1..256 (checked first) and cand_size above 64: SLG_ERR_UNSUPPORTED before the index (NULL here)"""
    from searchlite_amd import _native as N
    keep, args = _args(cand, nprobe)
    assert getattr(lib, name)(None, *args) == N.ERR_UNSUPPORTED
    assert word in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_UNSUPPORTED
    if word == b"cand_size":  # the message points to the calls that take a larger cand_size
        assert b"slg_vector_search_batch" in lib.slg_last_error() and b"approx" in lib.slg_last_error()
    assert _untouched(keep)


@pytest.mark.parametrize("name", SEARCH)
@pytest.mark.parametrize("cand,nprobe", [(1, 1), (5, 2), (64, 256), (33, 1)])
def test_valid_values_reach_the_index_check(lib, name, cand, nprobe):
    from searchlite_amd import _native as N
    keep, args = _args(cand, nprobe)
    assert getattr(lib, name)(None, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_INVALID
    assert _untouched(keep)


@pytest.mark.parametrize("name", SEARCH)
def test_null_clause_field_is_invalid(lib, name):
    from searchlite_amd import _native as N
    keep, args = _args()
    args[2] = None
    assert getattr(lib, name)(None, *args) == N.ERR_INVALID
    assert lib.slg_last_error() != b""


def test_cluster_and_fetch_on_a_null_index(lib):
    from searchlite_amd import _native as N
    d = (N.VectorListsDesc * 1)()
    assert lib.slg_index_cluster_vector_field(None, 0, C.addressof(d), 1) == N.ERR_INVALID
    assert b"index is NULL" in lib.slg_last_error()
    assert lib.slg_index_fetch_vector_lists(None, 0, 0, None, None, None, 0, 0) == N.ERR_INVALID
    assert b"index is NULL" in lib.slg_last_error()


# ---- train_centroids ----
def _blobs(rng, n, dim, k):
    centres = rng.standard_normal((k, dim)).astype(np.float32) * 4
    return (centres[rng.integers(0, k, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.3).astype(np.float32)


@pytest.mark.parametrize("metric", [0, 1])
def test_train_centroids_is_seeded_and_shaped(metric):
    from searchlite_amd.ivf import train_centroids
    x = _blobs(np.random.default_rng(5), 500, 9, 6)
    a = train_centroids(x, 6, metric, iters=4, seed=3)
    b = train_centroids(x.copy(), 6, metric, iters=4, seed=3)
    assert a.dtype == np.float32 and a.shape == (6, 9) and a.flags.c_contiguous
    assert a.tobytes() == b.tobytes()
    assert train_centroids(x, 6, metric, iters=4, seed=4).tobytes() != a.tobytes()
    assert np.isfinite(a).all()
    s = train_centroids(x, 6, metric, iters=2, seed=3, sample=100)
    assert s.shape == (6, 9) and s.tobytes() == train_centroids(x, 6, metric, iters=2, seed=3, sample=100).tobytes()
    if metric == 0:
        assert np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
        assert np.abs(np.linalg.norm(s.astype(np.float64), axis=1) - 1.0).max() <= 1e-6


@pytest.mark.parametrize("metric", [0, 1])
def test_train_centroids_clips_n_lists_to_the_rows(metric):
    from searchlite_amd.ivf import train_centroids
    x = _blobs(np.random.default_rng(6), 5, 4, 2)
    c = train_centroids(x, 9, metric, iters=3)
    assert c.shape == (5, 4) and np.isfinite(c).all()
    assert train_centroids(x, 9, metric, iters=2, sample=3).shape == (3, 4)


@pytest.mark.parametrize("metric", [0, 1])
def test_train_centroids_an_emptied_cluster_keeps_its_centroid(metric):
    """Four identical rows and three lists: the start picks three of them, every row goes to list 0 (ties: the lowest
    id), and lists 1 and 2 are empty from the first step on: they keep the centroid they started with."""
    from searchlite_amd.ivf import train_centroids
    x = np.tile(np.array([[3.0, 4.0]], np.float32), (4, 1))
    c = train_centroids(x, 3, metric, iters=5)
    want = np.array([0.6, 0.8], np.float32) if metric == 0 else np.array([3.0, 4.0], np.float32)
    assert c.shape == (3, 2) and not np.isnan(c).any()
    assert np.allclose(c, want, atol=1e-6)
    # and a start that loses a cluster on the way: the far row's cluster stays where it was when it emptied
    y = np.array([[1.0, 0.0], [1.0, 0.01], [0.0, 1.0]], np.float32)
    for seed in range(4):
        c = train_centroids(y, 3, metric, iters=4, seed=seed)
        assert c.shape == (3, 2) and np.isfinite(c).all()
