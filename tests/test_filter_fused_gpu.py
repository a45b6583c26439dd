"""GPU tests (-m gpu): the commit stage of the match chain in one launch - bf_siftmgr_commit_frame (k_commit_frame) - bit for bit against the two launches it
replaces, filter_frames_async + add_curr_to_residuals: EntryJ rows, the key side table, the row count, the frame result record and the valid flags.
(The combined surface-area + dense-verification launch this file was meant to hold as well did not meet its bar and is not in the library:
profiles/bundling_chain.md.)"""
import numpy as np
import pytest

from bundlefusion_amd.capi import ENTRYJ_DTYPE, _d2h, _h2d
from tests import filter_cases as fc

pytestmark = pytest.mark.gpu


def _commit_manager(gpu, n_images, mk, counts, seed, invalid=()):
    rng = np.random.default_rng(seed)
    allkeys = np.c_[rng.uniform(5, 630, n_images * mk), rng.uniform(5, 470, n_images * mk), rng.uniform(3, 12, n_images * mk),
                    rng.uniform(0.8, 3.0, n_images * mk)].astype(np.float32)
    mgr = gpu.capi.SiftManager(n_images, mk)
    descs = np.zeros((mk, 128), np.uint8)
    for i in range(n_images):
        mgr.add_image_host(allkeys[i * mk:(i + 1) * mk], descs)
        mgr.set_valid_image(i, 0 if i in invalid else 1)
    mgr.update_gpu_valid_images()
    cur = n_images - 1
    for p, cnt in enumerate(counts):
        idx = np.c_[p * mk + rng.integers(mk, size=fc.MAX_FILT), cur * mk + rng.integers(mk, size=fc.MAX_FILT)].astype(np.uint32)
        fc.check_indices(idx, n_images, mk)
        mgr.set_filt_matches(p, cnt, idx, np.zeros(fc.MAX_FILT, np.float32), np.eye(4), np.eye(4))
    return mgr, cur


def _frame_record(gpu, mgr):
    import ctypes as C
    p = C.c_void_p()
    gpu.capi.check(gpu.capi.lib.bf_siftmgr_get_frame_result_gpu(mgr._h, C.byref(p)))
    return _d2h(p.value, 16).view(np.int32).copy()


def _commit(gpu, mgr, cur, start, Kinv, fused):
    """one commit stage; returns everything it leaves: (rows, key pairs, row count, frame record, device valid flags, last matched frame)"""
    if fused:
        mgr.commit_frame(cur, start, cur + 1, Kinv)
    else:
        mgr.filter_frames_async(cur, start, cur + 1)
        mgr.add_curr_to_residuals(cur, start, cur + 1, Kinv)
    last, _ = mgr.sync_frame_result(cur)
    corr, ckeys = mgr.download_global_correspondences()
    valid = _d2h(mgr.valid_images_gpu(), 4 * (cur + 1)).view(np.int32).copy()
    return corr.tobytes(), ckeys.tobytes(), mgr.num_global_correspondences(), _frame_record(gpu, mgr).tobytes(), valid.tobytes(), last


def test_commit_frame_mixed_counts_and_a_frame_without_partner(gpu, oracle):
    Kinv = oracle.inverse44(fc.K)
    counts = (25, 0, 1, 25, 0, 7, 0)
    res = []
    for fused in (False, True):
        mgr, cur = _commit_manager(gpu, 8, 64, counts, 301)
        a = _commit(gpu, mgr, cur, 0, Kinv, fused)
        assert a[2] == sum(counts) and a[5] == 5                      # the last previous image with matches
        b = _commit(gpu, mgr, cur, 2, Kinv, fused)                    # startFrame = 2: the rows of images 2 .. 6 once more
        assert b[2] == sum(counts) + sum(counts[2:])
        for p in range(cur):                                          # no valid previous image: nothing is added, the count stays, the frame is invalid
            mgr.set_valid_image(p, 0)
        mgr.update_gpu_valid_images()
        c = _commit(gpu, mgr, cur, 0, Kinv, fused)
        assert c[2] == b[2] and c[:2] == b[:2] and c[5] == 0xFFFFFFFF
        rec = np.frombuffer(c[3], np.int32)
        assert rec[0] == -1 and rec[1] == 0 and rec[2] == b[2] and rec[3] == 64
        assert np.frombuffer(c[4], np.int32)[cur] == 0
        res.append((a, b, c))
    assert res[0] == res[1]


def test_commit_frame_crosses_the_capacity_inside_a_pair(gpu, oracle):
    """a 4-image manager holds 150 rows: 60 per frame -> 60, 120, 150 - the third call is cut five rows into its second pair - and 150"""
    Kinv = oracle.inverse44(fc.K)
    res = []
    for fused in (False, True):
        mgr, cur = _commit_manager(gpu, 4, 64, (25, 25, 10), 302)
        steps = [_commit(gpu, mgr, cur, 0, Kinv, fused) for _ in range(4)]
        assert [s[2] for s in steps] == [60, 120, 150, 150]
        res.append(steps)
    assert res[0] == res[1]


def test_commit_frame_more_than_1024_pairs(gpu, oracle):
    """1030 previous images of 16 keys (the global manager of a long stream): the block-scan form.  The last previous images have no matches and one with
    matches is invalid, so the last matched frame is neither the end of the range nor the last image with matches."""
    Kinv = oracle.inverse44(fc.K)
    n_prev = 1030
    rng = np.random.default_rng(303)
    counts = rng.choice([0, 0, 1, 3, 25], size=n_prev)
    counts[-7:] = 0; counts[-8] = 4; counts[-9] = 2
    mgr, cur = _commit_manager(gpu, n_prev + 1, 16, counts.tolist(), 303, invalid=(n_prev - 8, 5))
    total = int(counts.sum())
    poison = np.full(total * 32, 0xAB, np.uint8)
    import ctypes as C
    kp = C.c_void_p(); gpu.capi.check(gpu.capi.lib.bf_siftmgr_get_global_correspondence_keys_gpu(mgr._h, C.byref(kp)))
    res = []
    for fused in (False, True):
        mgr.set_global_correspondences(np.zeros(0, ENTRYJ_DTYPE))
        _h2d(mgr.global_correspondences_gpu(), poison); _h2d(kp.value, poison[:total * 8])
        r = _commit(gpu, mgr, cur, 0, Kinv, fused)
        assert r[2] == total and r[5] == n_prev - 9
        res.append(r)
    assert res[0] == res[1]
    corr = np.frombuffer(res[1][0], ENTRYJ_DTYPE)
    assert np.array_equal(corr["imgIdx_i"], np.repeat(np.arange(n_prev, dtype=np.uint32), counts)) and (corr["imgIdx_j"] == cur).all()
