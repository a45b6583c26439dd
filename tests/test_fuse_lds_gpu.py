"""GPU tests (-m gpu): key-frame fusion with the track search in LDS (k_fuse_to_global_lds) against the search in global memory (k_fuse_to_global,
bf_siftmgr_set_fuse_lds_limit(0)) and against the reference's host form (bf_siftmgr_fuse_to_global_host) on planted correspondence graphs.  Key
points as uint32 views, descriptors and counts bit for bit; fuse_error() == 0; fuse_path() tells which search ran."""
import ctypes as C

import numpy as np
import pytest

from bundlefusion_amd.capi import ENTRYJ_DTYPE, intrinsics_matrix

pytestmark = pytest.mark.gpu

K = intrinsics_matrix(583.0, 583.0, 319.5, 239.5)
OUTLIER, INVALID = 1, 2


def _chunk(gpu, oracle, nI, per, mk, corrs, seed):
    """a chunk manager of nI images with `per` random keys each and the correspondences corrs = [(i, a, j, b, kind)] (image i key a with image j key b;
    kind 0: consistent with the poses, OUTLIER: 0.1 m off, INVALID: invalidated) in list order; returns (manager, device poses, active key count)"""
    import torch
    from bundlefusion_amd.capi import lib, check, _h2d
    rng = np.random.default_rng(seed)
    Kinv = oracle.inverse44(K)
    loc = gpu.capi.SiftManager(nI + 1, mk)
    T = []
    for i in range(nI):
        M = np.eye(4, dtype=np.float32); M[:3, 3] = rng.normal(0, 0.05, 3).astype(np.float32); T.append(M)
    keys = []
    for i in range(nI):
        k = np.c_[rng.uniform(5, 630, per), rng.uniform(5, 470, per), rng.uniform(3, 12, per), rng.uniform(0.8, 3.0, per)].astype(np.float32)
        keys.append(k)
        loc.add_image_host(k, rng.integers(0, 255, (per, 128)).astype(np.uint8))
    packed = np.concatenate(keys)
    Tinv = [np.linalg.inv(t.astype(np.float64)) for t in T]
    corr, ck, active = [], [], set()
    for i, a, j, b, kind in corrs:
        assert i != j and a < per and b < per
        e = oracle.make_entry(packed, i * per + a, j * per + b, i, j, Kinv)
        wi = (T[i].astype(np.float64) @ np.r_[e["pos_i"].astype(np.float64), 1.0])[:3]
        e["pos_j"] = (Tinv[j] @ np.r_[wi, 1.0])[:3].astype(np.float32)
        if kind == OUTLIER:
            e["pos_j"] = e["pos_j"] + np.float32(0.1)
        elif kind == INVALID:
            e["imgIdx_i"] = 0xFFFFFFFF
        else:
            assert kind == 0
        if kind != INVALID:
            active.update((i * mk + a, j * mk + b))
        corr.append(e); ck.append((i * mk + a, j * mk + b))
    loc.set_global_correspondences(np.array(corr, dtype=ENTRYJ_DTYPE))
    p = C.c_void_p(); check(lib.bf_siftmgr_get_global_correspondence_keys_gpu(loc._h, C.byref(p)))
    _h2d(p.value, np.array(ck, np.uint32))
    return loc, torch.from_numpy(np.stack(T)).cuda(), len(active)


def _fuse3(gpu, oracle, loc, dT, gmax, limit=None):
    """fuse three times into one global manager - the LDS search (or what `limit` selects), the search in global memory, the host form - and hold the three
    key frames equal; returns (key points, descriptors, path of the first)"""
    Kinv = oracle.inverse44(K)
    glob = gpu.capi.SiftManager(4, gmax)
    if limit is not None:
        loc.set_fuse_lds_limit(limit)
    loc.fuse_to_global(glob, K, dT.data_ptr(), Kinv)
    path = loc.fuse_path()
    loc.set_fuse_lds_limit(0)
    loc.fuse_to_global(glob, K, dT.data_ptr(), Kinv)
    assert loc.fuse_path() == 0
    loc.fuse_to_global(glob, K, dT.data_ptr(), Kinv, host=True)
    assert loc.fuse_error() == 0
    assert glob.num_images() == 3
    (k0, d0), (k1, d1), (k2, d2) = (glob.download_image(i) for i in range(3))
    assert len(k0) == len(k1) == len(k2), (len(k0), len(k1), len(k2))
    assert np.array_equal(k0.view(np.uint32), k1.view(np.uint32)) and np.array_equal(d0, d1), "LDS search differs from the search in global memory"
    assert np.array_equal(k0.view(np.uint32), k2.view(np.uint32)) and np.array_equal(d0, d2), "LDS search differs from the host form"
    return k0, d0, path


def _random_corrs(rng, nI, per, ncorr):
    """the generator of test_fuse_to_global_device_equals_host_on_random_graphs: 15 % outliers, 7 % invalidated"""
    out = []
    for _ in range(ncorr):
        i, j = sorted(rng.choice(nI, 2, replace=False).tolist())
        a, b = int(rng.integers(per)), int(rng.integers(per))
        r = rng.random()
        out.append((i, a, j, b, OUTLIER if r < 0.15 else INVALID if r < 0.22 else 0))
    return out


def test_cliques_over_eleven_images(gpu, oracle):
    """11 images x 8 keys, every feature seen in all images and matched between every two of them: 55 correspondences and 110 list entries per component -
    the longest search, and the start key is listed by every other key of its component"""
    rng = np.random.default_rng(1)
    corrs = [(i, f, j, f, 0) for f in range(8) for i in range(11) for j in range(i + 1, 11)]
    corrs = [corrs[q] for q in rng.permutation(len(corrs))]
    assert len(corrs) == 8 * 55
    loc, dT, active = _chunk(gpu, oracle, 11, 8, 16, corrs, 1)
    assert active == 88
    k, _, path = _fuse3(gpu, oracle, loc, dT, 64)
    assert len(k) == 8 and path == 1


def test_one_path_through_all_keys(gpu, oracle):
    """3 images x 40 keys joined into ONE path of 119 correspondences whose order along the path is unrelated to the key order: the labelling needs many
    sweeps and the search is as deep as the graph"""
    rng = np.random.default_rng(2)
    order = [rng.permutation(40) for _ in range(3)]
    seq = [(n % 3, int(order[n % 3][n // 3])) for n in range(120)]
    corrs = [(seq[n][0], seq[n][1], seq[n + 1][0], seq[n + 1][1], 0) for n in range(119)]
    corrs = [corrs[q] for q in rng.permutation(119)]
    loc, dT, active = _chunk(gpu, oracle, 3, 40, 64, corrs, 2)
    assert active == 120
    k, _, path = _fuse3(gpu, oracle, loc, dT, 64)
    assert len(k) == 1 and path == 1


def test_triangles_reenter_their_start_key_and_repeated_neighbours(gpu, oracle):
    """triangles in all six orders of their correspondences (the second key of the search lists the start key, which is not marked yet: it is entered again),
    and pairs of keys joined by three correspondences, one of them an outlier (a key's list holds one neighbour several times)"""
    import itertools
    corrs = []
    for f, perm in enumerate(itertools.permutations(range(3))):
        tri = [(0, f, 1, f, 0), (1, f, 2, f, 0), (0, f, 2, f, 0)]
        corrs += [tri[q] for q in perm]
    for f in range(6, 10):
        corrs += [(0, f, 1, f, 0), (0, f, 1, f, OUTLIER if f % 2 else 0), (0, f, 1, f, 0)]
    loc, dT, active = _chunk(gpu, oracle, 3, 10, 16, corrs, 3)
    assert active == 18 + 8
    k, _, path = _fuse3(gpu, oracle, loc, dT, 64)
    assert len(k) == 10 and path == 1


def test_outliers_and_invalidated_correspondences(gpu, oracle):
    """every correspondence an outlier or invalidated but one: one track; all outliers: no track at all, and a key frame of 0 keys from all three forms"""
    base = [(i, f, j, f, OUTLIER if (i + j + f) % 2 else INVALID) for f in range(5) for i in range(4) for j in range(i + 1, 4)]
    assert base[0][4] == OUTLIER
    kept = list(base); kept[0] = kept[0][:4] + (0,)        # the first entry of the first start key's list: the search takes it before any other route to that key
    loc, dT, _ = _chunk(gpu, oracle, 4, 5, 16, kept, 4)
    k, _, path = _fuse3(gpu, oracle, loc, dT, 64)
    assert len(k) == 1 and path == 1
    loc, dT, _ = _chunk(gpu, oracle, 4, 5, 16, [c[:4] + (OUTLIER,) for c in base], 5)
    k, _, path = _fuse3(gpu, oracle, loc, dT, 64)
    assert len(k) == 0 and path == 1


def test_over_full_key_frame(gpu, oracle):
    """(6, 64, 64, 32, 250) of the random-graph test: more tracks than the key frame holds - keys by depth, descriptors in track order"""
    rng = np.random.default_rng(102)
    loc, dT, _ = _chunk(gpu, oracle, 6, 64, 64, _random_corrs(rng, 6, 64, 250), 102)
    k, _, path = _fuse3(gpu, oracle, loc, dT, 32)
    assert len(k) == 32 and path == 1


def test_limit_at_the_active_key_count(gpu, oracle):
    """the limit at exactly the number of keys with a valid correspondence: the LDS search; one less: the search in global memory; same key frame"""
    rng = np.random.default_rng(7)
    loc, dT, active = _chunk(gpu, oracle, 5, 12, 16, _random_corrs(rng, 5, 12, 40), 7)
    assert 20 < active <= 60
    k1, d1, path = _fuse3(gpu, oracle, loc, dT, 64, limit=active)
    assert path == 1
    k0, d0, path = _fuse3(gpu, oracle, loc, dT, 64, limit=active - 1)
    assert path == 0
    assert len(k1) >= 1 and np.array_equal(k1.view(np.uint32), k0.view(np.uint32)) and np.array_equal(d1, d0)


def test_benchmark_shape(gpu, oracle):
    """11 images x 1024 keys, 1300 random correspondences: the chunk manager of the frame loop, nearly full"""
    rng = np.random.default_rng(8)
    loc, dT, active = _chunk(gpu, oracle, 11, 1024, 1024, _random_corrs(rng, 11, 1024, 1300), 8)
    assert active > 2000
    k, _, path = _fuse3(gpu, oracle, loc, dT, 1024)
    assert len(k) > 500 and path == 1
