"""The planted voxel-update cases (tests/voxel_update_cases.py) without a GPU: the oracle against the float64 restatement (tests/voxel_update_ref.py) on every
planted volume, script and parameter set; the proof that the volumes hold the cases they are named after; and that no voxel had to be excluded.

Bounds.  Weights, validity and alpha: equal.  Colour: equal after integrations and after de-integrations at w <= 1024; above that within 1 LSB (a float32 and a
float64 quotient fall on different sides of a tie only when 1 / (2 (w - 1)) approaches the float32 error of the quotient, 254 x 2^-24 x a few operations).
sdf: within 1e-5 x m_truncation, the project's single-operator bound (SDF_TOL of tests/test_tsdf_fast_gpu.py); the figures printed here show how far inside
it the reference itself sits.
"""
import numpy as np
import pytest

from tests import voxel_update_cases as vc
from tests import voxel_update_ref as ref

SDF_TOL = 1e-5
SDF_TOL_LONG = 1e-4
EXACT_COLOUR_UP_TO = 1024


def compare_with_restatement(what, vox, st, seen, info, p, sdf_tol=SDF_TOL, report=True):
    """vox: a volume's voxels (oracle or product); st: the restatement's state; seen: largest weight every voxel was de-integrated at (0: never).
    -> {planted weight: (voxels, max |dsdf| / truncation, colour bytes differing)}"""
    w = vox["weight"].astype(np.float64)
    ds = np.abs(vox["sdf"].astype(np.float64) - st.sdf) / float(p.m_truncation)
    dc = np.abs(vox["color"][:, :3].astype(np.int64) - st.colour.astype(np.int64))
    rows = {}
    for pw in np.unique(info["weight"]):
        m = info["weight"] == pw
        rows[int(pw)] = (int(m.sum()), float(ds[m].max()), int((dc[m] != 0).sum()))
    if report:
        print("%s: planted weight -> (voxels, max |dsdf| / truncation, colour bytes differing; -1: not planted): %s" % (what, rows))
    assert np.array_equal(w, st.weight), "%s: %d weights differ" % (what, int((w != st.weight).sum()))
    assert np.array_equal(vox["color"][:, 3].astype(np.int64), st.alpha), what + ": alpha"
    low = seen <= EXACT_COLOUR_UP_TO
    assert not dc[low].any(), "%s: %d colour bytes differ after integrations / de-integrations at w <= %d" % (what, int((dc[low] != 0).sum()), EXACT_COLOUR_UP_TO)
    assert dc.max(initial=0) <= 1, "%s: colour off by %d" % (what, int(dc.max()))
    assert ds.max() <= sdf_tol, "%s: sdf off by %.3g x truncation" % (what, float(ds.max()))
    return rows


@pytest.mark.parametrize("cfg", list(vc.CONFIGS))
def test_oracle_equals_the_float64_restatement_on_every_planted_volume(oracle, cfg):
    worst = 0.0
    for name in vc.scripts_for(cfg):
        vol = vc.Volume(oracle, cfg)
        info = vc.plant(vol)
        st = ref.State(vol.osc.voxels())
        seen = np.zeros(len(st.weight))
        log = vol.run_oracle(vc.SCRIPTS[name], st, seen)
        rows = compare_with_restatement("%s / %s" % (cfg, name), vol.osc.voxels(), st, seen, info, vol.p)
        worst = max(worst, max(r[1] for r in rows.values()))
        print("%s / %s: voxels updated per operator %s" % (cfg, name, [(k, f, int(ok.sum())) for k, f, _, _, ok in log]))
    print("%s: largest oracle-to-float64 sdf distance %.3g x truncation (bound %.0e)" % (cfg, worst, SDF_TOL))


def test_emptied_blocks_are_collected(oracle):
    vol = vc.Volume(oracle, "default")
    info = vc.plant(vol, emptied=True)
    st = ref.State(vol.osc.voxels())
    seen = np.zeros(len(st.weight))
    before = vol.osc.num_allocated()
    vol.run_oracle(vc.SCRIPTS["deintegrate"], st, seen)
    compare_with_restatement("emptied", vol.osc.voxels(), st, seen, info, vol.p, report=False)
    vol.garbage_collect()
    left = set(vc.hash_map(vol.osc))
    freed = before - vol.osc.num_allocated()
    print("emptied: %d of %d blocks planted to be emptied, %d collected" % (len(info["emptied_keys"]), before, freed))
    assert not (left & info["emptied_keys"]) and freed >= len(info["emptied_keys"]) >= vc.FACTS["emptied_blocks"]


def test_organic_script_on_the_oracle(oracle):
    vol = vc.Volume(oracle, "default", alloc=[])
    st = vc.organic_ref(vol)
    vox = vol.osc.voxels()
    assert np.array_equal(vox["weight"].astype(np.float64), st.weight) and st.weight.max() == 300
    ds = float(np.abs(vox["sdf"].astype(np.float64) - st.sdf).max()) / float(vol.p.m_truncation)
    dc = np.abs(vox["color"][:, :3].astype(np.int64) - st.colour.astype(np.int64))
    print("organic: %d blocks, weights up to %d, oracle-to-float64 sdf distance %.3g x truncation after %d integrations, %d colour bytes differ"
          % (vol.osc.num_allocated(), int(st.weight.max()), ds, vc.ORGANIC_INTEGRATIONS, int((dc != 0).sum())))
    assert ds <= SDF_TOL_LONG and not dc.any()
    vol.run_oracle(vc.organic_ops("de"))
    vol.garbage_collect()
    assert vc.is_empty(vol.osc.hash(), vol.osc.heap(), vol.osc.heap_counter(), vol.osc.voxels(), vol.p)


@pytest.mark.parametrize("cfg", list(vc.CONFIGS))
def test_the_volumes_hold_the_cases_they_are_named_after(oracle, cfg):
    F = vc.FACTS
    vol = vc.Volume(oracle, cfg)
    info = vc.plant(vol)
    p, cam = vol.p, vol.cam
    planted = vol.osc.voxels().copy()
    cap = int(p.m_integrationWeightMax)
    # every planted state is reachable: integer weights with alpha 255, or the all-zero voxel
    live = planted["weight"] > 0
    assert (planted["color"][live, 3] == 255).all() and not planted[~live].view(np.uint8).any() and (planted["weight"] == np.round(planted["weight"])).all()
    assert planted["weight"].max() <= cap and (planted["color"][:, :3] <= 254).all()
    up = info["updated_by_A"]
    # per class and operator: enough voxels, in all 8 z-slices of a block (where the band is narrower than a block: in every slice the operator reaches), and in
    # both halves of the kernels' voxel pairs
    n_slices = len(np.unique(info["local_z"][up]))
    assert n_slices == (8 if cfg not in ("coarse", "narrow") else n_slices) and n_slices >= 3
    counts = {}
    for name, cls, names in (("weight", info["weight"], None), ("sdf", info["sdf_class"], vc.SDF_CLASSES), ("colour", info["colour_class"], vc.COLOUR_CLASSES)):
        for v in np.unique(cls[cls >= 0]):
            m = up & (cls == v)
            counts[(name, names[v] if names else int(v))] = int(m.sum())
            if name == "weight" or m.sum() >= 8 * 20:
                assert len(np.unique(info["local_z"][m])) == n_slices and len(np.unique(info["local_z"][m] & 1)) == 2, (name, v)
    print("%s: %d blocks, (\"de\" / \"in\", A, identity) updates %d voxels; per class: %s" % (cfg, vol.osc.num_allocated(), int(up.sum()), counts))
    assert sorted(k[1] for k in counts if k[0] == "weight") == vc.weights_for(p)
    assert min(v for k, v in counts.items() if k[0] == "weight") >= F["per_weight_class"][cfg]
    if cfg == "default":
        assert min(v for k, v in counts.items() if k[0] == "sdf") >= F["per_sdf_class"] and min(v for k, v in counts.items() if k[0] == "colour") >= F["per_colour_class"]
        # the cancelling voxels: float32 numerators of 0, and non-zero ones below 2^-60 (divStored's literal division; the sign of a zero quotient)
        n = info["numerator"][up & (info["weight"] > 0)]
        sel = up & (info["weight"] > 0)
        n_in = info["sample_A"][sel] + (planted["sdf"] * planted["weight"]).astype(np.float32)[sel]
        zero, tiny = int((n == 0).sum()), int(((n != 0) & (np.abs(n) < 2.0 ** -60)).sum())
        neg_zero = int(((n == 0) & np.signbit(n)).sum())
        zero_in = int((n_in == 0).sum())
        can = up & np.isin(info["sdf_class"], (vc.S_CANCEL_DE, vc.S_CANCEL_IN))
        by_w = {int(w): (int((can & (info["weight"] == w)).sum()), int((can & info["cancel_found"] & (info["weight"] == w)).sum())) for w in np.unique(info["weight"][can])}
        print("default: de-integration numerators: %d are 0 (%d of them -0.0), %d non-zero below 2^-60; integration numerators that are 0: %d; cancelling voxels planted / found per weight: %s"
              % (zero, neg_zero, tiny, zero_in, by_w))
        assert zero >= F["numerator_zero"] and neg_zero > 0 and neg_zero < zero and tiny >= F["numerator_tiny"] and zero_in >= F["numerator_zero"]
        assert by_w[2][1] >= F["numerator_zero"] and sum(v[1] for w, v in by_w.items() if w > 2) >= F["numerator_zero"]
        # ties of the de-integration colour quotient under frame A
        cA = np.array(vc.COL_A[:3], np.float64)
        t = up & (info["colour_class"] == vc.C_TIE)
        q = (planted["color"][t, :3].astype(np.float64) * planted["weight"][t, None] - cA) / (planted["weight"][t, None] - 1.0)
        half = np.abs(q - np.floor(q) - 0.5) == 0
        ties = dict(negative=int((half & (q < 0)).sum()), low=int((half & (q > 0) & (q < 5)).sum()), below_254=int((half & (q > 249.5) & (q < 254.5)).sum()),
                    from_254=int((half & (q >= 254.5)).sum()), all=int(half.sum()), at_w3=int(half[planted["weight"][t] == 3].sum()), at_w5=int(half[planted["weight"][t] == 5].sum()))
        print("default: colour channels with a half-integer de-integration quotient:", ties)
        assert ties["negative"] >= F["ties_negative"] and ties["low"] >= F["ties_low"] and ties["below_254"] >= F["ties_below_254"] and ties["from_254"] >= F["ties_from_254"]
        assert ties["at_w3"] > 0 and ties["at_w5"] > 0
    if cap < 70000:
        # the cap binds: voxels at the cap change and keep their weight; a de-integration then leaves them at cap - 1 - it is no inverse
        st = ref.State(planted)
        vol.run_oracle(vc.SCRIPTS["integrate"], st)
        after = vol.osc.voxels().copy()
        at_cap = up & (info["weight"] == cap)
        changed = at_cap & (after["sdf"] != planted["sdf"])
        assert (after["weight"][at_cap] == cap).all() and changed.sum() >= F["cap_binds"]
        vol.run_oracle(vc.SCRIPTS["deintegrate"], st)
        back = vol.osc.voxels()
        assert (back["weight"][at_cap] == cap - 1).all()
        print("%s: %d voxels at the cap, %d change sdf under the integration and keep the weight; the de-integration leaves them at %d" % (cfg, int(at_cap.sum()), int(changed.sum()), cap - 1))
    # the truncation bound: the slice the edge depths were found for is updated one step below the bound, and not on it or above it
    if "edge_on" in vc.scripts_for(cfg):
        e = vc.edge_depths(p, vc.CONFIGS[cfg][1])
        idx, coord, _ = ref.voxel_index(vol.osc.hash())
        got = {}
        for side, frame in ((-1, "E_BELOW"), (0, "E_ON"), (1, "E_ABOVE")):
            D, k = e[side]
            sdf = np.abs(np.float32(D) - vc.slice_z(p, k))
            steps = int(sdf.view(np.int32)) - int(vc.trunc32(p, D).view(np.int32))
            assert steps == side and vol.frames[frame][0][0, 0] == D
            _, ok, _, _ = ref.sample(vol.osc.hash(), vc.IDENT, vol.frames[frame][0], True, cam, p)
            sl = coord[:, 2] == k
            nb = (coord[:, 2] == (k + 1 if vc.slice_z(p, k) < D else k - 1))          # the neighbouring slice on the side of the surface is inside the bound
            got[frame] = (float(D), k, int((ok & sl).sum()), int(sl.sum()), int((ok & nb).sum()))
            assert ((ok & sl).sum() == 0 if side >= 0 else (ok & sl).sum() >= F["edge_slice"]) and (ok & nb).sum() >= F["edge_slice"]
        print("%s: edge frames: name -> (depth, slice, voxels of the slice updated, allocated, updated in the next slice inwards): %s" % (cfg, got))
    if "maxdist" in vc.scripts_for(cfg):
        n_at = int(ref.sample(vol.osc.hash(), vc.IDENT, vol.frames["MAXD"][0], True, cam, p)[1].sum())
        n_below = int(ref.sample(vol.osc.hash(), vc.IDENT, vol.frames["MAXD_BELOW"][0], True, cam, p)[1].sum())
        print("%s: depth == m_maxIntegrationDistance updates %d voxels, one float32 step below %d" % (cfg, n_at, n_below))
        assert n_at == 0 and n_below >= F["edge_slice"]
        assert vol.frames["MAXD"][0][0, 0] == np.float32(p.m_maxIntegrationDistance) > vol.frames["MAXD_BELOW"][0][0, 0]


@pytest.mark.parametrize("cfg", list(vc.CONFIGS))
def test_no_voxel_lies_near_an_image_bound(oracle, cfg):
    """Nothing is excluded: under every pose used, no voxel of any block the scripts allocate projects within 1e-3 px (five times the largest band the fast-contract
    tests use at this image size) of the bounds -1 and W (H) that decide whether it is in the image."""
    vol = vc.Volume(oracle, cfg)
    for name in vc.scripts_for(cfg):
        vol.run_oracle(vc.SCRIPTS[name])
    idx, coord, key = ref.voxel_index(vol.osc.hash())
    worst = np.inf
    for pname in vc.poses_for(cfg):
        T = vc.POSES[pname]
        pr = ref.project(coord, key, T, vol.cam, vol.p)
        front = pr["z"] > 0
        d = np.minimum(np.minimum(np.abs(pr["hx"] + 1.0), np.abs(pr["hx"] - vc.W)), np.minimum(np.abs(pr["hy"] + 1.0), np.abs(pr["hy"] - vc.H)))[front]
        print("%s / %s: %d voxels, smallest distance of a projection to an image bound %.3g px" % (cfg, pname, int(front.sum()), float(d.min())))
        assert front.all()
        worst = min(worst, float(d.min()))
    assert worst > vc.FACTS["bound_margin_px"], "a voxel projects within %.3g px of an image bound: move the principal point or the pose" % worst
