"""GPU parity tests (-m gpu): HIP SIFT detection (csrc/sift.hip) against the CPU oracle, bit for bit (tolerance 0), on the planted images of tests/sift_cases.py -
where the per-level caps of k_keys_finalize and k_reshape bind, where the two LimitFeatureCount passes decide differently, at the boundary of the scale gate,
under depth maps of another size, next to the image borders, on octaves of a few pixels, and from one frame to the next on the same detector.
tests/test_sift_cases_cpu.py proves on the oracle that every image holds its case."""
import ctypes as C

import numpy as np
import pytest

from tests import sift_cases as sc

pytestmark = pytest.mark.gpu

MAX_KEYS = 192                  # every case has fewer features (the CPU test bounds them), so rows are left over for the sentinel
KEY_SENTINEL, DESC_SENTINEL = np.float32(-7.25), np.uint8(0xA5)
_expected = {}


def expected(oracle, name, max_features=MAX_KEYS):
    """the oracle's result of a case, computed once"""
    if (name, max_features) not in _expected:
        _, I, d, kw = sc.case(name)
        n, keys, descs, _ = oracle.sift_run(I, d, max_features=max_features, **kw)
        _expected[(name, max_features)] = (n, keys, descs, oracle.sift_stages(I, d, **kw))
    return _expected[(name, max_features)]


def make_detector(gpu, name, max_keys=MAX_KEYS):
    _, I, d, kw = sc.case(name)
    return gpu.capi.Sift(I.shape[1], I.shape[0], d.shape[1], d.shape[0], max_keys=max_keys, **kw)


def run(sift, name):
    """one frame into sentinel-filled outputs: (n, all key rows, all descriptor rows)"""
    import torch
    _, I, d, _ = sc.case(name)
    keys = torch.full((sift.max_keys, 4), float(KEY_SENTINEL), device="cuda")
    descs = torch.full((sift.max_keys, 128), int(DESC_SENTINEL), dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), -99, dtype=torch.int32, device="cuda")
    sift.run(torch.from_numpy(I.copy()).cuda(), torch.from_numpy(d.copy()).cuda(), keys, descs, cnt)
    return int(cnt.item()), keys.cpu().numpy(), descs.cpu().numpy()


def assert_equals_oracle(sift, got, want, name):
    n, keys, descs = got
    on, okeys, odescs, st = want
    cnts = sift.debug_counts()
    print(name, "n", n, "level0", cnts["level0"], "level1", cnts["level1"])
    assert cnts["level0"] == st["level0"].tolist(), name                       # after LimitFeatureCount(0), k_keys_finalize
    assert cnts["level1"] == st["level1"].tolist(), name                       # after the reshape and LimitFeatureCount(1), k_reshape
    assert cnts["num_raw"] == st["level0"].sum()
    assert n == on, name
    assert np.array_equal(keys[:n].view(np.uint32), okeys.view(np.uint32)), name
    assert np.array_equal(descs[:n], odescs), name
    assert np.all(keys[n:].view(np.uint32) == KEY_SENTINEL.view(np.uint32)) and np.all(descs[n:] == DESC_SENTINEL), name      # rows n.. are not touched


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_bit_exact(gpu, oracle, name):
    sift = make_detector(gpu, name)
    assert_equals_oracle(sift, run(sift, name), expected(oracle, name), name)
    sift.close()


@pytest.mark.parametrize("name", ["cap64", "cap72x88", "coarse96_oct3"])
def test_every_pyramid_level_of_the_small_images(gpu, oracle, name):
    """64 x 64 (octave 3 is 8 x 8: a 33-tap blur clamps on every side of the tile), 72 x 88 (no multiple of the tile), 96 x 80 (12 x 10)"""
    _, I, _, _ = sc.case(name)
    sift = make_detector(gpu, name)
    run(sift, name)
    for o in range(4):
        for a in range(6):
            assert np.array_equal(sift.debug_level(o, a).view(np.uint32), oracle.sift_pyramid_level(I, o, a).view(np.uint32)), (name, o, a)
    sift.close()


@pytest.mark.parametrize("name", sc.CAP_CASES)
def test_cap_cases_do_not_depend_on_arrival_order(gpu, oracle, name):
    """three frames on one detector: the candidates arrive through atomicAdd in any order, the sort of k_keys_finalize alone makes `the first fmax` a fact of the image"""
    sift = make_detector(gpu, name)
    want = expected(oracle, name)
    for _ in range(3):
        assert_equals_oracle(sift, run(sift, name), want, name)
    sift.close()


@pytest.mark.parametrize("sequence", [["cap64", "coarse64", "constant", "cap64"],                         # busy, sparse, empty, busy: 64 x 64
                                      ["mixed_scale0", "cap128_oct1", "cap128_oct0", "mixed_scale0"]])     # other slots busy from frame to frame: 128 x 96
def test_state_is_recycled_between_frames(gpu, oracle, sequence):
    """candCount, ticket and the error flag are reset on the device for the next frame: every frame equals the oracle's result for its own image"""
    cases = [sc.case(n) for n in sequence]
    assert all(c[1].shape == cases[0][1].shape and c[2].shape == cases[0][2].shape and c[3] == cases[0][3] for c in cases)       # one detector serves them all
    sift = make_detector(gpu, sequence[0])
    for name in sequence:
        assert_equals_oracle(sift, run(sift, name), expected(oracle, name), name)
    sift.close()


def test_a_frame_after_too_many_keypoints_is_clean(gpu, oracle):
    sift = make_detector(gpu, "cap64", max_keys=16)
    for name, n_want in (("coarse64", 2), ("cap64", -1), ("coarse64", 2), ("constant", 0), ("cap64", -1)):
        n, keys, descs = run(sift, name)
        on, okeys, odescs, st = expected(oracle, name, 16)
        assert n == on == n_want, name
        cnts = sift.debug_counts()
        assert cnts["level0"] == st["level0"].tolist() and cnts["level1"] == st["level1"].tolist(), name
        if n >= 0:
            assert np.array_equal(keys[:n].view(np.uint32), okeys.view(np.uint32)) and np.array_equal(descs[:n], odescs), name
            assert np.all(keys[n:].view(np.uint32) == KEY_SENTINEL.view(np.uint32)) and np.all(descs[n:] == DESC_SENTINEL), name
    sift.close()


def test_more_raw_keys_than_2048(gpu, oracle):
    """The one image beyond 160 x 152: 3487 raw keys at 640 x 480 with threshold 0.  k_orientation ran 2048 workgroups whatever the image, one per raw key: the
    keys behind the 2048th kept `no orientation` and the reshape dropped them."""
    sift = make_detector(gpu, "many_keys640", max_keys=4800)
    want = expected(oracle, "many_keys640", 4800)
    assert want[0] > 2048
    assert_equals_oracle(sift, run(sift, "many_keys640"), want, "many_keys640")
    sift.close()


def _create(gpu, w, h):
    handle = C.c_void_p()
    rc = gpu.capi.lib.bf_sift_create(w, h, w, h, 150, C.c_float(0.1), C.c_float(4.0), C.c_float(3.0), 1024, C.byref(handle))
    return rc, handle, gpu.capi.lib.bf_last_error().decode()


@pytest.mark.parametrize("size", [(1280, 960), (648, 480)])
def test_sizes_beyond_the_raw_key_list_are_refused(gpu, size):
    """The raw key list and the LDS arrays of k_reshape hold 6144 keys = the per-level caps of 640 x 480 summed; a larger image could deliver more with
    featureCountThreshold 0.  Only the refusal is tested: nothing is launched."""
    rc, handle, msg = _create(gpu, *size)
    assert rc == -1 and not handle.value                                       # BF_ERR_INVALID_ARG
    assert "bf_sift_create" in msg and "too large" in msg and "6144" in msg, msg


def test_coordinates_beyond_16_bits_are_refused(gpu):
    rc, handle, msg = _create(gpu, 65544, 64)                                  # candidates are packed as row << 16 | col
    assert rc == -1 and not handle.value and "16 bits" in msg, msg


def test_the_pipeline_size_is_still_accepted(gpu):
    rc, handle, msg = _create(gpu, 640, 480)
    assert rc == 0 and handle.value, msg
    assert gpu.capi.lib.bf_sift_destroy(handle) == 0
