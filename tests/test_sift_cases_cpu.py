"""CPU tests (-m "not gpu"): the planted SIFT images of tests/sift_cases.py hold the cases they are named after - asserted on the oracle's own stages
(tests/oracle_api.py sift_stages), so that an image that stops driving its branch fails here instead of passing silently on the device - and the
oracle's raw key sets against a float64 numpy restatement of the pyramid and of the extremum / contrast / edge tests."""
import numpy as np
import pytest

from tests import sift_cases as sc


_facts = {}


def facts(oracle, name):
    if name not in _facts:
        _, I, d, kw = sc.case(name)
        st = oracle.sift_stages(I, d, **kw)
        n, keys, descs, lv = oracle.sift_run(I, d, **kw)
        assert n == st["n"] and lv.tolist() == st["level1"].tolist()
        raw = oracle.sift_detect(I, d, kw.get("depth_min", sc.DEPTH_MIN), kw.get("depth_max", sc.DEPTH_MAX))
        H, W = I.shape
        fmax = np.repeat([sc.fmax_of(W >> o, H >> o) for o in range(4)], 3)
        cap = np.repeat([sc.cand_cap_of(W >> o, H >> o) for o in range(4)], 3)
        print("%-28s %3dx%-3d depth %3dx%-3d %s\n    raw %s l0 %s rs %s l1 %s n %d" % (name, W, H, d.shape[1], d.shape[0], kw, st["uncapped"].tolist(), st["level0"].tolist(),
                                                                                       st["reshaped"].tolist(), st["level1"].tolist(), n))
        _facts[name] = dict(st, I=I, d=d, kw=kw, keys=keys, descs=descs, raw=raw, fmax=fmax, cap=cap, W=W, H=H)
    return _facts[name]


def straddlers(f, slot):
    """raw keys of a slot with two orientations of which exactly the first fits under fmax (scale gate open)"""
    n = f["n_ori"][slot]
    before = np.concatenate([[0], np.cumsum(n)[:-1]])
    return [i for i in range(len(n)) if n[i] == 2 and before[i] == f["fmax"][slot] - 1]


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_is_in_the_supported_range(oracle, name):
    """every case: at most 160 x 152, and no slot's extrema come near the candidate buffer (beyond it the surviving candidates depend on the order of arrival)"""
    f = facts(oracle, name)
    assert f["W"] <= 160 and f["H"] <= 152 and f["W"] % 8 == 0 and f["H"] % 8 == 0 and f["W"] >= 64 and f["H"] >= 64
    assert np.all(f["uncapped"] <= 0.8 * f["cap"]), (f["uncapped"], f["cap"])
    assert f["n"] <= 160                                                    # tests/test_sift_cases_gpu.py gives every detector 192 rows and checks the rest
    assert np.all(f["reshaped"] <= f["fmax"]) and np.all(f["level0"] <= f["fmax"])


@pytest.mark.parametrize("name,slot,npad", [("cap64", 0, 128), ("cap64_straddle", 0, 128), ("cap72x88", 0, 128), ("cap128_oct1", 3, 64), ("cap128_oct0", 0, 256)])
def test_raw_cap_and_reshape_cap_bind(oracle, name, slot, npad):
    f = facts(oracle, name)
    fmax = f["fmax"][slot]
    assert f["uncapped"][slot] > fmax == f["level0"][slot]                    # (a) k_keys_finalize keeps the first fmax of the sorted candidates
    assert npad // 2 < f["uncapped"][slot] <= npad                            # the bitonic sort's padded size
    n = f["n_ori"][slot]
    assert len(n) == fmax and (n == 2).sum() >= 1 and n.sum() > fmax          # (b) keys left over: the capped walk of k_reshape binds
    assert f["reshaped"][slot] == f["level1"][slot] == fmax
    assert f["kw"]["min_key_scale"] == 0.0 and f["kw"]["feature_count_threshold"] == 0
    if name == "cap128_oct1":
        assert slot // 3 == 1 and 1 <= f["uncapped"][2] <= 64                 # the capped slot lies in octave 1, beside a slot of npad 64
    if name == "cap128_oct0":
        assert fmax == 61


def test_a_two_orientation_key_straddles_the_cap(oracle):
    assert straddlers(facts(oracle, "cap64"), 0) == []                        # the plain image: 18 keys fill the 32 places exactly ...
    f = facts(oracle, "cap64_straddle")
    assert f["uncapped"][0] == facts(oracle, "cap64")["uncapped"][0] - 2      # ... with the depth gone under its first two keys the walk shifts by one
    assert [tuple(k) for k in facts(oracle, "cap64")["raw"][0][:2]] == sc.CAP64_KNOCKED_KEYS
    assert len(straddlers(f, 0)) == 1 and len(straddlers(facts(oracle, "cap72x88"), 0)) == 1
    for name in ("cap64_straddle", "cap72x88"):
        f = facts(oracle, name)
        i = straddlers(f, 0)[0]
        col, row = f["raw"][0][i]
        # the level's last feature is that key's first orientation; the key in front of it is another one
        assert f["keys"][31, 0] == col + 0.5 and f["keys"][31, 1] == row + 0.5 and tuple(f["keys"][30, :2]) != tuple(f["keys"][31, :2])


def test_a_straddling_key_in_front_of_a_later_slot(oracle):
    """mixed: slot 3 is full with a straddling key and slot 5 follows - a second orientation that is not cut lands on slot 5's first feature (in a list that
    ends with the capped slot it falls behind the end and nothing shows)"""
    f = facts(oracle, "mixed_scale0")
    assert len(straddlers(f, 3)) == 1 and f["reshaped"][3] == f["fmax"][3] and f["level1"][5] > 0
    assert f["n_ori"][0].sum() > f["fmax"][0] == f["reshaped"][0] and f["level1"][1] > 0


def test_more_raw_keys_than_2048(oracle):
    _, I, d, kw = sc.case("many_keys640")
    st = oracle.sift_stages(I, d, capacity=2048, **kw)
    assert st["level0"].sum() > 2048 and st["level0"].sum() <= 6144 and np.all(st["uncapped"][:3] <= 0.8 * sc.cand_cap_of(640, 480))
    assert (np.concatenate(st["n_ori"])[2048:] > 0).sum() > 1000                  # keys behind the 2048th with an orientation
    assert 2048 < st["n"] <= 4800
    print("many_keys640 raw %s l0 %s rs %s n %d" % (st["uncapped"].tolist(), st["level0"].tolist(), st["reshaped"].tolist(), st["n"]))


def test_limit0_against_limit1(oracle):
    base = facts(oracle, "mixed_scale0")                                      # threshold 0
    raw, rs = base["level0"], base["reshaped"]
    assert raw.sum() == sc.MIXED_RAW_TOTAL and raw[0] == sc.MIXED_RAW0 and rs.sum() == sc.MIXED_RS_TOTAL and rs[0] == sc.MIXED_RS0
    assert (raw > 0).sum() >= 5 and base["uncapped"][0] > raw[0]
    f = facts(oracle, "mixed_limit1_drops")                                   # limit 0 keeps what limit 1 drops
    assert f["level0"].tolist() == raw.tolist() and f["level1"][0] == 0 and f["level1"][1] == 0 and f["reshaped"][0] > 0 and f["reshaped"][1] > 0 and f["level1"][2] > 0
    f = facts(oracle, "mixed_both_drop")                                      # both drop, limit 1 one slot more
    assert f["level0"][0] == 0 and f["level0"][1] == 0 and f["level0"][2] > 0 and f["level1"][2] == 0 and f["reshaped"][2] > 0 and f["level1"][3] > 0
    f = facts(oracle, "mixed_limit0_boundary")                                # total - levelNum[0] == threshold: `>` keeps the slot
    assert f["kw"]["feature_count_threshold"] == raw.sum() - raw[0] and f["level0"].tolist() == raw.tolist()
    f = facts(oracle, "mixed_limit0_below_boundary")
    assert f["level0"][0] == 0 and f["level0"][1:].tolist() == raw[1:].tolist()
    f = facts(oracle, "mixed_limit1_boundary")
    assert f["kw"]["feature_count_threshold"] == rs.sum() - rs[0] and f["level1"].tolist() == rs.tolist()
    f = facts(oracle, "mixed_limit1_below_boundary")
    assert f["level0"].tolist() == raw.tolist() and f["level1"][0] == 0 and f["level1"][1:].tolist() == rs[1:].tolist()
    f = facts(oracle, "mixed_defaults")
    assert f["level1"][0] == 0 and f["level1"][1] == 0 and f["level1"][2:].tolist() == rs[2:].tolist()


def test_min_key_scale_cases(oracle):
    base = facts(oracle, "mixed_scale0")
    assert (base["level1"] > 0).sum() >= 3
    f = facts(oracle, "mixed_scale_boundary")                                 # sigma * keyLocScale >= min_key_scale keeps slot 0 at equality
    assert f["kw"]["min_key_scale"] == sc.LEVEL0_SCALE and f["level1"].tolist() == base["level1"].tolist()
    assert np.float32(f["keys"][0, 2]) == np.float32(sc.LEVEL0_SCALE)         # the scale the detector itself reports for slot 0
    f = facts(oracle, "mixed_scale_above_boundary")                           # one float32 step above: slot 0 goes, slot 1 stays
    assert f["level1"][0] == 0 and f["level0"][0] > 0 and f["level1"][1:].tolist() == base["level1"][1:].tolist()
    f = facts(oracle, "mixed_scale41")
    assert f["level1"][:4].tolist() == [0, 0, 0, 0] and f["level1"].sum() > 0 and np.all(f["level0"] == base["level0"])


@pytest.mark.parametrize("name", ["depth128_half", "depth128_wider", "depth64_rows_only", "depth128_inf_right"])
def test_depth_of_another_size(oracle, name):
    f = facts(oracle, name)
    I, d, W, H = f["I"], f["d"], f["W"], f["H"]
    dH, dW = d.shape
    assert (dW, dH) != (W, H)
    full = oracle.sift_detect(I, np.ones_like(d))                             # the same image, every depth valid
    keys = f["keys"]
    assert f["n"] > 20 and np.all(np.isfinite(keys[:, 3])) and np.all(keys[:, 3] >= sc.DEPTH_MIN) and np.all(keys[:, 3] <= sc.DEPTH_MAX)
    # the depth each key reports is the map's value at roundf(pos * (dW - 1) / (W - 1)), float64 here; the ramp makes every neighbour another value
    px = keys[:, 0].astype(np.float64) * (dW - 1) / (W - 1); py = keys[:, 1].astype(np.float64) * (dH - 1) / (H - 1)
    frac = np.maximum(np.abs(px - np.floor(px) - 0.5), np.abs(py - np.floor(py) - 0.5))
    sure = frac > 1e-4                                                        # float32 rounding of the product cannot move these across .5
    assert sure.mean() > 0.9
    ix, iy = np.floor(px + 0.5).astype(int), np.floor(py + 0.5).astype(int)
    assert np.array_equal(keys[sure, 3], d[iy[sure], ix[sure]])
    wrong = d[np.minimum(iy + 1, dH - 1), ix]                                 # one off: another value
    assert np.all(wrong[sure] != keys[sure, 3])
    # each band crosses keypoints: extrema of the all-valid image whose look-up pixel falls into it
    hit = {"inf": 0, "near": 0, "far": 0}
    for slot in range(12):
        for col, row in full[slot]:
            dx, dy = sc.depth_lookup(col, row, slot // 3, W, H, dW, dH)
            v = d[dy, dx]
            hit["inf"] += v == -np.inf; hit["near"] += np.isfinite(v) and v < sc.DEPTH_MIN; hit["far"] += v > sc.DEPTH_MAX
    print(name, hit)
    if name == "depth128_inf_right":
        assert hit["inf"] > 10 and f["n"] == 61 and np.all(keys[:, 0] * (dW - 1) / (W - 1) < 39.5 + 1e-3)
    else:
        assert min(hit.values()) >= 2, hit
        assert (sc.key_slots(f["level1"]) >= 3).sum() >= (3 if W == 128 else 1)   # keys of octave 1: keyLocScale 2 in the look-up
    assert f["uncapped"].sum() < oracle.sift_stages(I, np.ones_like(d), **f["kw"])["uncapped"].sum()


def test_keys_near_every_border_and_on_coarse_octaves(oracle):
    f = facts(oracle, "borders")
    slot = sc.key_slots(f["level1"])
    octave = slot // 3
    sigma = f["keys"][:, 2] / (1 << octave)                                    # scale = keyLocScale * sigma
    x = (f["keys"][:, 0] - 0.5) / (1 << octave) + 0.5; y = (f["keys"][:, 1] - 0.5) / (1 << octave) + 0.5     # position on the key's own level
    w = f["W"] >> octave; h = f["H"] >> octave
    win = 3.0 * sigma
    # the orientation window [x - win, x + win] is clamped by fmaxf(1.5, .) / fminf(w - 1.5, .)
    left, right, top, bottom = x - win < 1.5, x + win > w - 1.5, y - win < 1.5, y + win > h - 1.5
    fine = octave == 0
    assert (left & fine).sum() >= 1 and (right & fine).sum() >= 1 and (top & fine).sum() >= 1 and (bottom & fine).sum() >= 1
    assert (left & top).sum() >= 1 and (right & bottom).sum() >= 1            # two windows clamped on both axes
    assert (octave >= 2).sum() >= 1
    c = facts(oracle, "coarse64")
    assert c["level1"].nonzero()[0].tolist() == [8] and c["uncapped"].sum() == 1
    c = facts(oracle, "coarse96_oct3")
    assert c["level1"].nonzero()[0].tolist() == [9] and c["uncapped"].sum() == 1          # octave 3: 12 x 10 pixels, every 33-tap blur clamps on all sides
    assert facts(oracle, "constant")["uncapped"].sum() == 0 and facts(oracle, "constant")["n"] == 0


def test_candidate_counts_cover_the_sort_sizes(oracle):
    """cnt = 0, 1..64 (npad 64), 65..128 (npad 128), just over a power of two, and 129..256 among the slots of the cases"""
    counts = np.concatenate([facts(oracle, n)["uncapped"] for n in sc.CASE_NAMES])
    assert (counts == 0).any() and (counts == 1).any() and ((counts > 1) & (counts <= 64)).any() and ((counts > 64) & (counts <= 128)).any() and ((counts > 128) & (counts <= 256)).any()
    assert any(c - p <= 9 for c in counts for p in (64, 128) if c > p), counts[counts > 64]


# ---------------------------------------------------------------------------------------------------- float64 restatement
def _taps64(sigma):
    """CreateFilterKernel in float64: 2 ceil(4 sigma - 0.5) + 1 taps, clamped to 5..33, normalised"""
    sz = int(np.ceil(4.0 * sigma - 0.5))
    sz = 16 if 2 * sz + 1 > 33 else (2 if 2 * sz + 1 < 5 else sz)
    x = np.arange(-sz, sz + 1, dtype=np.float64)
    k = np.exp(-0.5 * x * x / (sigma * sigma))
    return k / k.sum()


def _blur64(img, k):
    pad = len(k) // 2
    t = np.pad(img, pad, mode="edge")
    t = np.stack([np.convolve(r, k[::-1], mode="valid") for r in t])
    return np.stack([np.convolve(c, k[::-1], mode="valid") for c in t.T]).T


def _pyramid64(I):
    f = np.float32
    sigma0 = f(1.6) * f(2.0) ** f(1 / 3)
    sigmak = f(2.0) ** f(1 / 3)
    dsigma0 = sigma0 * np.sqrt(f(1.0) - f(1.0) / (sigmak * sigmak))
    sa = sigma0 * f(2.0) ** f(-1 / 3)
    sig = [float(np.sqrt(sa * sa - f(0.25)))] + [float(dsigma0 * sigmak ** f(i)) for i in range(5)]
    octs = []
    for o in range(4):
        lev = [_blur64(I.astype(np.float64), _taps64(sig[0]))] if o == 0 else [octs[-1][3][::2, ::2]]
        for j in range(5):
            lev.append(_blur64(lev[-1], _taps64(sig[j + 1])))
        octs.append(lev)
    return octs


def _classify64(dog_prev, dog, dog_next, margin=1e-5):
    """float64 decision per pixel of a DoG level: +1 key, 0 no key, -1 undecided (some test within `margin` of its boundary while no other test rejects clearly)"""
    h, w = dog.shape
    out = np.zeros((h, w), np.int8)
    thr, tedge = 0.02 / 3, (10.0 + 1) ** 2 / 10.0
    for r in range(1, h - 2):
        for c in range(1, w - 2):
            v = dog[r, c]
            m = [abs(v) - thr]                                              # contrast
            nb = np.concatenate([dog_prev[r - 1:r + 2, c - 1:c + 2].ravel(), dog_next[r - 1:r + 2, c - 1:c + 2].ravel(), np.delete(dog[r - 1:r + 2, c - 1:c + 2].ravel(), 4)])
            m.append(max(v - nb.max(), nb.min() - v))                       # strict extremum of its 26 neighbours
            fxx = dog[r, c - 1] + dog[r, c + 1] - 2 * v; fyy = dog[r - 1, c] + dog[r + 1, c] - 2 * v
            fxy = 0.25 * (dog[r + 1, c + 1] + dog[r - 1, c - 1] - dog[r + 1, c - 1] - dog[r - 1, c + 1])
            t1 = fxx * fyy - fxy * fxy; t2 = (fxx + fyy) ** 2
            m += [t1, tedge * t1 - t2]                                      # edge test
            if min(m) <= -margin:
                continue
            out[r, c] = 1 if min(m) >= margin else -1
    return out


def test_raw_keys_against_float64_extrema(oracle):
    """Not resting on the oracle's own arithmetic: the pyramid, the DoG levels and the strict 26-neighbour extremum, contrast and edge tests restated in float64
    numpy.  Pixels with a float64 margin below 1e-5 on a test are left out; they stay under 5 % of the keys, and every blob gives a key."""
    I, spec = sc.blob_field()
    H, W = I.shape
    raw = oracle.sift_detect(I, np.ones_like(I))
    st = oracle.sift_stages(I, np.ones_like(I), min_key_scale=0.0, feature_count_threshold=0)
    assert np.array_equal(st["uncapped"], [len(r) for r in raw])              # no slot is capped: the raw lists are the whole extremum sets
    octs = _pyramid64(I)
    for o in range(4):
        for a in range(6):
            assert np.abs(oracle.sift_pyramid_level(I, o, a) - octs[o][a]).max() < 2e-6, (o, a)
    total = undecided = 0
    near_blob = np.zeros(len(spec), int)
    for o in range(4):
        dog = [octs[o][a + 1] - octs[o][a] for a in range(5)]
        for j in range(1, 4):
            slot = o * 3 + j - 1
            cls = _classify64(dog[j - 1], dog[j], dog[j + 1])
            got = np.zeros(cls.shape, bool)
            for col, row in raw[slot]:
                got[row, col] = True
            decided = cls >= 0
            assert np.array_equal(got[decided], cls[decided] == 1), (slot, np.argwhere(decided & (got != (cls == 1))))
            total += int((cls != 0).sum()); undecided += int((cls == -1).sum())      # an undecided pixel is one that no test rejects clearly: a possible key
            for row, col in np.argwhere(cls == 1):
                x, y = (col + 0.5) * (1 << o), (row + 0.5) * (1 << o)
                for i, (cx, cy, b) in enumerate(spec):
                    near_blob[i] += (x - cx) ** 2 + (y - cy) ** 2 <= (2 << o) ** 2
    print("float64 extrema: %d keys, %d undecided; keys per blob %s" % (total, undecided, near_blob.tolist()))
    assert total >= len(spec) and undecided < 0.05 * total
    assert np.all(near_blob >= 1), near_blob
