"""Planted inputs of the descriptor matcher (k_match of siftmgr.hip), shared by tests/test_match_edge_cpu.py (the cases hold what they are named after; the
oracle against the compiled reference matcher) and tests/test_match_edge_gpu.py (k_match against the oracle, bit for bit).  Pure numpy, fixed seeds: both
tests see the same bytes.

A case is one image pair: `prev` [n1, 128] u8 and `cur` [n2, 128] u8, the key-store stride `max_keys`, the two thresholds, and `expect`: the (previous key,
current key) pairs the matcher must return, in ascending current-key order, BEFORE the cap of 128 (the matcher keeps the first 128 of that order and reports
the full count).  Cases that share one current image (the same bytes) and the same launch parameters go into one manager: layouts() groups them.

Descriptors are SIFT-like rows: |normal|, L2-normalised, times a scale, rounded to bytes.  Two unrelated rows have a cosine of about 0.64, a distance of about
0.88: they fail dist_max = 0.7.  A partner is a copy of one row at a chosen key of the other image, with optional noise of a few counts per byte.  At scale 512
about half of the planted dot products reach 2^18, where the distance clamps to exactly 0 (equal distances for the sort); the cases that need positive, distinct
distances use scale 480."""
import numpy as np

MAX_RAW = 128
DIST_MAX, RATIO_MAX = 0.7, 0.8

KEY_COUNTS_CUR = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1009, 1024)      # either side of the 16-key MFMA tile, the 64-key slab, the 256-column
KEY_COUNTS_PREV = (1, 16, 17, 64, 65, 1009, 1024)                             # compaction pass and the bound of 1024 keys
CAP_CASES = ((300, 127), (300, 128), (300, 129), (300, 300), (1024, 200), (1024, 1024))      # (keys on both sides, partners)
STRIDES = ((16, (1, 15, 16)), (1000, (993, 1000)))                            # (max_keys, key counts on both sides)
TIE_RATIO = 1.25
THRESH_RANK = 10                     # the planted match (in distance order) whose own distance becomes dist_max
FRAME_COUNTS = (64, 0, 300, 17, 1024, 129)


def descriptors(rng, n, scale=512):
    d = np.abs(rng.normal(size=(n, 128)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.clip(np.floor(d * scale + 0.5), 0, 255).astype(np.uint8)


def noisy(rng, d, noise):
    if noise == 0:
        return d.copy()
    return np.clip(d.astype(int) + rng.integers(-noise, noise + 1, d.shape), 0, 255).astype(np.uint8)


def _pick(rng, n, m):
    """m distinct keys of n, sorted, key 0 and key n - 1 among them.  m == 1 (one side has a single key, so one partner is all there can be): the last key."""
    assert 1 <= m <= n
    if m == 1:
        return np.array([n - 1])
    return np.sort(np.r_[0, rng.permutation(np.arange(1, n - 1))[:m - 2], n - 1]).astype(np.int64)


def _pairs(rows, cols):
    p = np.c_[np.asarray(rows, np.int64), np.asarray(cols, np.int64)].reshape(-1, 2)
    return p[np.argsort(p[:, 1], kind="stable")]


def _case(name, family, prev, cur, expect, max_keys=1024, dist_max=DIST_MAX, ratio_max=RATIO_MAX, **extra):
    c = dict(name=name, family=family, prev=prev, cur=cur, expect=_pairs(*np.asarray(expect, np.int64).reshape(-1, 2).T), max_keys=max_keys,
             dist_max=dist_max, ratio_max=ratio_max)
    c.update(extra)
    return c


def _planted_prev(rng, cur, n1, cols, scale=512, noise=2):
    """a previous image of n1 keys with one partner (a random row, key 0 and the last key among them) for each of the given current keys"""
    rows = rng.permutation(_pick(rng, n1, len(cols)))
    prev = descriptors(rng, n1, scale)
    prev[rows] = noisy(rng, cur[cols], noise)
    return prev, _pairs(rows, cols)


# ------------------------------------------------------------------------------------------------ the families
def key_count_cases():
    """84 pairs, min(n1, n2, 100) partners each with noise +-2; the previous images of one n2 share the current image"""
    out = []
    for n2 in KEY_COUNTS_CUR:
        cur = descriptors(np.random.default_rng([1, n2]), n2)
        for n1 in KEY_COUNTS_PREV:
            rng = np.random.default_rng([2, n1, n2])
            cols = _pick(rng, n2, min(n1, n2, 100))
            prev, pairs = _planted_prev(rng, cur, n1, cols)
            out.append(_case("keys %d x %d" % (n1, n2), "key_counts", prev, cur, pairs))
    return out


def _cap_columns(rng, n, m):
    if (n, m) == (300, 129):            # 128 partners in the first compaction pass, the 129th in the second
        return np.r_[_pick(rng, 256, 128), n - 1]
    if (n, m) == (1024, 200):           # 50 per pass, 5 keys apart: position 128 is the 29th partner of the third pass, lane 12 of its third wave
        cols = np.concatenate([256 * p + 5 * np.arange(50) for p in range(4)])
        cols[-1] = n - 1
        return cols
    return _pick(rng, n, m)


def cap_cases():
    out = []
    curs = {n: descriptors(np.random.default_rng([3, n]), n) for n in (300, 1024)}
    for n, m in CAP_CASES:
        rng = np.random.default_rng([4, n, m])
        cols = _cap_columns(rng, n, m)
        assert len(cols) == m and len(set(cols.tolist())) == m and cols[0] == 0 and cols[-1] == n - 1
        prev, pairs = _planted_prev(rng, curs[n], n, cols)
        out.append(_case("cap %d x %d, %d partners" % (n, n, m), "cap", prev, curs[n], pairs))
    # what the two special layouts promise
    c129, c200 = out[2]["expect"][:, 1], out[4]["expect"][:, 1]
    assert c129[127] < 256 <= c129[128]
    assert [int(((c200 >= 256 * p) & (c200 < 256 * (p + 1))).sum()) for p in range(4)] == [50, 50, 50, 50]
    w = c200[(c200 >= 512) & (c200 < 768)]
    assert c200[128] == w[28] and (c200[128] - 512) // 64 == (w[27] - 512) // 64 and (c200[128] - 512) % 64 > (w[27] - 512) % 64      # crossed mid-wave
    return out


def equal_distance_case():
    """every row of both images is a permutation of ONE byte multiset and the 100 partners are exact copies: every planted dot product, hence every distance,
    is the same, so the order of the output is the sort's tie rule alone (ascending current key)"""
    rng = np.random.default_rng([5])
    base = descriptors(rng, 1)[0]
    prev = np.stack([rng.permutation(base) for _ in range(200)])
    cur = np.stack([rng.permutation(base) for _ in range(200)])
    cols = _pick(rng, 200, 100)
    rows = rng.permutation(_pick(rng, 200, 100))
    cur[cols] = prev[rows]
    return [_case("equal distances 200 x 200", "equal", prev, cur, _pairs(rows, cols))]


def tie_cases():
    """dot-product ties that decide the match.  Descriptor A sits at previous keys 35 and 129 and at current key 50: column 50 sees two equal best rows and takes
    129 (its key ((r >> 2) & 31, r) is (0, 129) against (8, 35)).  Descriptor B sits at current keys 33 and 64 and at previous key 70: row 70 takes column 64
    ((c & 31, c) is (0, 64) against (1, 33)).  Best equals second best there, so the pair passes the ratio test only where ratio_max > 1 (scale 480: the
    distance is positive)."""
    rng = np.random.default_rng([6])
    prev, cur = descriptors(rng, 200, 480), descriptors(rng, 200, 480)
    A, B = descriptors(rng, 2, 480)
    prev[35] = prev[129] = cur[50] = A
    cur[33] = cur[64] = prev[70] = B
    return [_case("ties, ratio_max 1.25", "ties", prev, cur, [(129, 50), (70, 64)], ratio_max=TIE_RATIO, lowest_index_rule=[(35, 50), (70, 33)]),
            _case("ties, ratio_max 0.8", "ties", prev, cur, [])]


def threshold_base_case():
    """20 partners at scale 480 with noise +-6: positive distances, pairwise distinct (asserted by the CPU test)"""
    rng = np.random.default_rng([7])
    cur = descriptors(rng, 200, 480)
    prev, pairs = _planted_prev(rng, cur, 200, _pick(rng, 200, 20), 480, 6)
    return _case("thresholds 200 x 200", "thresholds", prev, cur, pairs)


def threshold_variants(case, idx, dist, rank=THRESH_RANK):
    """`idx`, `dist`: the matcher's distance-sorted output for `case` (key indices inside the two images).  dist_max = the distance of match `rank` itself: the
    strict `<` drops it and every match farther away; dist_max = the next float: it is kept."""
    dist = np.asarray(dist, np.float32)
    assert len(dist) > rank + 1 and (np.diff(dist) > 0).all(), "the threshold case needs distinct distances"
    d = dist[rank]
    return [dict(case, name=case["name"] + ", dist_max = d[%d]" % rank, dist_max=float(d), expect=_pairs(*np.asarray(idx[:rank], np.int64).T)),
            dict(case, name=case["name"] + ", dist_max = next(d[%d])" % rank, dist_max=float(np.nextafter(d, np.float32(np.inf))),
                 expect=_pairs(*np.asarray(idx[:rank + 1], np.int64).T))]


def saturated_and_zero_cases():
    """90 x 85 keys with 30 partners.  With one all-zero key on each side the partners are returned (a zero key matches nothing).  With one all-255 key on each
    side as well NOTHING is returned: the saturated key has the largest dot product against every key of the other image, every row and column verdict points at
    it, and the mutual check removes every pair; the saturated pair itself has best and second best beyond 2^18 (both distances 0) and fails the ratio test."""
    out = []
    for sat in (False, True):
        rng = np.random.default_rng([8])
        cur = descriptors(rng, 85)
        prev, pairs = _planted_prev(rng, cur, 90, _pick(rng, 85, 30))
        free_r = [r for r in range(1, 89) if r not in set(pairs[:, 0].tolist())]
        free_c = [c for c in range(1, 84) if c not in set(pairs[:, 1].tolist())]
        cur = cur.copy()
        prev[free_r[0]] = 0; cur[free_c[0]] = 0
        if sat:
            prev[free_r[5]] = 255; cur[free_c[7]] = 255
        out.append(_case("saturated and zero keys" if sat else "zero keys", "saturated", prev, cur, [] if sat else pairs, planted=pairs))
    return out


def stride_cases():
    """the key-count builder at other key-store strides: the index pairs are prev * max_keys + r, cur * max_keys + c"""
    out = []
    for mk, counts in STRIDES:
        for n2 in counts:
            cur = descriptors(np.random.default_rng([9, mk, n2]), n2)
            for n1 in counts:
                rng = np.random.default_rng([10, mk, n1, n2])
                prev, pairs = _planted_prev(rng, cur, n1, _pick(rng, n2, min(n1, n2, 100)))
                out.append(_case("stride %d: %d x %d" % (mk, n1, n2), "strides", prev, cur, pairs, max_keys=mk))
    return out


def all_cases():
    """every case whose expectation does not depend on computed distances (the threshold variants are derived from the base case: threshold_variants)"""
    return key_count_cases() + cap_cases() + equal_distance_case() + tie_cases() + [threshold_base_case()] + saturated_and_zero_cases() + stride_cases()


# ------------------------------------------------------------------------------------------------ the six-image manager of the frame-range tests
def frame_images():
    """six images of FRAME_COUNTS keys; image i holds noisy copies (+-2) of the first n_i descriptors of one pool in an order of its own, so any two non-empty
    images have min(n_a, n_b) partners: 129 x 300 and 129 x 1024 meet the cap, 17 and 64 do not"""
    rng = np.random.default_rng([11])
    pool = descriptors(rng, 1024)
    return [noisy(rng, pool[rng.permutation(n)], 2) for n in FRAME_COUNTS]


# ------------------------------------------------------------------------------------------------ layout and bounds
def check_bounds(images, max_keys, pairs=()):
    """before anything is uploaded: every image fits its slot of the key store (so no key the matcher reads and no index it writes lies outside the store), and
    every expected key index names a key of its image"""
    assert 16 <= max_keys <= 1024
    for d in images:
        assert d.dtype == np.uint8 and d.ndim == 2 and d.shape[1] == 128 and len(d) <= max_keys, "image does not fit its slot of the key store"
    for prev, cur, p in pairs:
        p = np.asarray(p, np.int64).reshape(-1, 2)
        assert p.size == 0 or (p.min() >= 0 and p[:, 0].max() < len(prev) and p[:, 1].max() < len(cur)), "expected key index outside its image"
    return images


def expected_output(case, prev_slot, cur_slot):
    """(count, the kept index pairs as the manager numbers them) of a case whose previous image sits in slot prev_slot and whose current image in cur_slot; the
    kept pairs are in ascending current-key order (the distance sort is the matcher's: compare as a set, or through the oracle)"""
    e = case["expect"]
    kept = e[:MAX_RAW]
    return len(e), np.c_[prev_slot * case["max_keys"] + kept[:, 0], cur_slot * case["max_keys"] + kept[:, 1]].astype(np.uint32)


def layouts(cases):
    """managers: the cases grouped by (max_keys, dist_max, ratio_max, bytes of the current image), in first-seen order.  Each layout: max_keys, dist_max,
    ratio_max, cur, cases (slot p holds cases[p]["prev"], the current image sits in slot len(cases))."""
    groups = {}
    for c in cases:
        key = (c["max_keys"], c["dist_max"], c["ratio_max"], c["cur"].tobytes())
        g = groups.setdefault(key, dict(max_keys=c["max_keys"], dist_max=c["dist_max"], ratio_max=c["ratio_max"], cur=c["cur"], cases=[]))
        g["cases"].append(c)
    out = list(groups.values())
    for g in out:
        check_bounds([c["prev"] for c in g["cases"]] + [g["cur"]], g["max_keys"], [(c["prev"], c["cur"], c["expect"]) for c in g["cases"]])
    return out
