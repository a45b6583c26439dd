"""GPU tests (-m gpu) of the four voxel-update kernels on the planted volumes of tests/voxel_update_cases.py: flat frames, so that a voxel's sample does not depend
on the pixel it projects into and EVERY voxel is compared - no band around pixel boundaries, nothing excluded (tests/test_voxel_update_cases_cpu.py proves that no
voxel lies within 1e-3 px of an image bound either).

  exact contract   k_update_col (serial) and k_update_batch_col (one run_batch): every script bit for bit against the oracle, on colFast's shared-reciprocal
                   quotients and, with BF_TSDF_EXACT_DIV=1, on colExact's literal divisions;
  fast contract    k_update_apx (serial) and k_update_batch_apx: table, heap and every weight equal the oracle's; sdf within SDF_TOL = 1e-5 x m_truncation of the
                   float64 restatement (tests/voxel_update_ref.py; the CPU file measures the oracle's own distance from it: up to 7e-7 under the identity and the
                   translation, 4.5e-6 under the rotation at 2 m, where the float32 camera-space z that both contracts share carries most of it); colour equal
                   to the oracle's after integrations and after de-integrations at w <= 1024 (a non-tie is at least 1 / (2 (w - 1)) >= 4.9e-4 away from a tie,
                   against the kernel's bias of 2^-12 plus its quotient error of 7e-5), within 1 LSB above; batched = serial bit for bit.

Measured on MI355X: profiles/voxel_update_cases.md.
"""
import numpy as np
import pytest

from bundlefusion_amd.capi import FREE_ENTRY

from tests import voxel_update_cases as vc
from tests import voxel_update_ref as ref
from tests.test_tsdf_gpu import assert_same_state

pytestmark = pytest.mark.gpu

SDF_TOL = 1e-5          # x m_truncation: one script on identical state (tests/test_tsdf_fast_gpu.py)
SDF_TOL_LONG = 1e-4     # x m_truncation: the organic script.  A 2-ulp step per integration grows by about n / 2 steps over n integrations in the worst case: 300
                        # integrations at |sdf| <= 0.12 give 2e-6 m, below the 6e-6 m this allows
EXACT_COLOUR_UP_TO = 1024

CASES = [(cfg, name) for cfg in vc.CONFIGS for name in vc.scripts_for(cfg)] + [("default", "emptied")]
FORMS = ("serial", "batch")


def _build(gpu, oracle, cfg, name):
    """-> (volume planted identically in the oracle and on the device, info, the planted records, the script)"""
    vol = vc.Volume(oracle, cfg, gpu=gpu)
    info = vc.plant(vol, emptied=name == "emptied")
    return vol, info, vol.osc.voxels().copy(), vc.SCRIPTS["deintegrate" if name == "emptied" else name]


def _run(vol, ops, form):
    (vol.run_serial if form == "serial" else vol.run_batch)(ops)


def _untouched(what, vox, planted, info):
    m = info["weight"] >= 0
    assert np.array_equal(vox[m].view(np.uint8), planted[m].view(np.uint8)), what + ": an operator that updates nothing changed a planted voxel"


@pytest.mark.parametrize("exact_div", [0, 1])
@pytest.mark.parametrize("cfg,name", CASES)
def test_exact_contract_equals_the_oracle_bit_for_bit(gpu, oracle, monkeypatch, cfg, name, exact_div):
    if exact_div:
        monkeypatch.setenv("BF_TSDF_EXACT_DIV", "1")          # read when a scene is created: every block takes colExact's literal `/`
    ref_state = None
    for form in FORMS:
        vol, info, planted, ops = _build(gpu, oracle, cfg, name)
        assert vol.gs.arith() == "exact"
        assert_same_state(vol.gs, vol.osc, "%s / %s planted:" % (cfg, name))
        _run(vol, ops, form)
        vol.run_oracle(ops)
        assert_same_state(vol.gs, vol.osc, "%s / %s %s:" % (cfg, name, form))
        if name == "emptied":
            before = vol.osc.num_allocated()
            vol.garbage_collect()
            assert_same_state(vol.gs, vol.osc, "%s / %s %s + GC:" % (cfg, name, form))
            assert before - vol.osc.num_allocated() >= len(info["emptied_keys"]) >= vc.FACTS["emptied_blocks"]
        if name == "nothing":
            _untouched("%s %s" % (name, form), vol.gs.download()[3], planted, info)


def _compare_fast(what, g, vol, st, seen, info, sdf_tol=SDF_TOL):
    """g: the product's download under the fast contract; the oracle ran the same script.  -> {planted weight: (voxels, max |dsdf| / truncation, colour bytes differing)}"""
    gh, gheap, gcnt, gvox = g
    osc, p = vol.osc, vol.p
    oh, ovox = osc.hash(), osc.voxels()
    ds = np.abs(gvox["sdf"].astype(np.float64) - st.sdf) / float(p.m_truncation)
    dc = np.abs(gvox["color"][:, :3].astype(np.int64) - ovox["color"][:, :3].astype(np.int64))
    rows = {}
    for pw in np.unique(info["weight"]):
        m = info["weight"] == pw
        rows[int(pw)] = (int(m.sum()), float(ds[m].max()), int((dc[m] != 0).sum()))
    print("%s: planted weight -> (voxels, max |dsdf| / truncation to the float64 restatement, colour bytes differing from the oracle; -1: not planted): %s" % (what, rows))
    assert gcnt == osc.heap_counter(), what + ": heap counter"
    for f in ("pos", "ptr", "offset"):
        assert np.array_equal(gh[f], oh[f]), what + ": hash." + f
    assert np.array_equal(gheap, osc.heap()), what + ": heap"
    assert np.array_equal(gvox["weight"], ovox["weight"]), "%s: %d weights differ" % (what, int((gvox["weight"] != ovox["weight"]).sum()))
    assert np.array_equal(gvox["color"][:, 3], ovox["color"][:, 3]), what + ": alpha"
    low = seen <= EXACT_COLOUR_UP_TO
    assert not dc[low].any(), "%s: %d colour bytes differ after integrations / de-integrations at w <= %d" % (what, int((dc[low] != 0).sum()), EXACT_COLOUR_UP_TO)
    assert dc.max(initial=0) <= 1, "%s: colour off by %d LSB" % (what, int(dc.max()))
    assert ds.max() <= sdf_tol, "%s: sdf off by %.3g x truncation" % (what, float(ds.max()))
    return rows, dc


@pytest.mark.parametrize("cfg,name", CASES)
def test_fast_contract_against_the_oracle_and_the_float64_restatement(gpu, oracle, cfg, name):
    out = {}
    for form in FORMS:
        vol, info, planted, ops = _build(gpu, oracle, cfg, name)
        vol.gs.set_arith("fast")
        assert vol.gs.arith() == "fast"
        _run(vol, ops, form)
        if name == "emptied":
            vol.gs.garbage_collect()
        out[form] = vol.gs.download()
        if form == "serial":          # one oracle and one float64 run serve both launch forms
            st = ref.State(planted)
            seen = np.zeros(len(planted))
            vol.run_oracle(ops, st, seen)
            if name == "emptied":
                vol.osc.garbage_collect()
            keep = vol
        rows, dc = _compare_fast("%s / %s %s" % (cfg, name, form), out[form], keep, st, seen, info)
        if name == "nothing":
            _untouched("%s %s" % (name, form), out[form][3], planted, info)
        if (cfg, name, form) == ("default", "deintegrate", "serial"):
            # the kernel's comment claims its biased nearest-even conversion equals roundf "for w < 2000"
            clean = [w for w in sorted(rows) if w > 0 and rows[w][2] == 0]
            dirty = [w for w in sorted(rows) if w > 0 and rows[w][2] != 0]
            print("de-integration colours under the fast contract: all equal to the oracle's at the planted weights %s; differing at %s; largest weight below the first difference: %s"
                  % (clean, dirty, max([w for w in clean if not dirty or w < dirty[0]], default=None)))
    a, b = out["serial"], out["batch"]
    assert a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), "batched and serial tables differ"
    assert np.array_equal(a[3].view(np.uint8), b[3].view(np.uint8)), "%d voxels differ between the batched and the serial run" % int(
        (a[3].view(np.uint8).reshape(len(a[3]), -1) != b[3].view(np.uint8).reshape(len(b[3]), -1)).any(axis=1).sum())


@pytest.fixture(scope="module")
def organic(oracle):
    """the organic script on the oracle and in float64, once: the state after the 300 integrations"""
    vol = vc.Volume(oracle, "default", alloc=[])
    st = vc.organic_ref(vol)
    return vol, st, (vol.osc.hash().copy(), vol.osc.heap().copy(), vol.osc.heap_counter(), vol.osc.voxels().copy())


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_organic_script_300_integrations_and_back_to_the_empty_volume(gpu, oracle, organic, arith):
    ovol, st, (oh, oheap, ocnt, ovox) = organic
    vol = vc.Volume(oracle, "default", gpu=gpu, alloc=[])
    vol.gs.set_arith(arith)
    vol.run_batch(vc.organic_ops("in"))
    gh, gheap, gcnt, gvox = vol.gs.download()
    assert gcnt == ocnt and np.array_equal(gheap, oheap)
    for f in ("pos", "ptr", "offset"):
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(gvox["weight"], ovox["weight"]) and gvox["weight"].max() == vc.ORGANIC_INTEGRATIONS
    ds = float(np.abs(gvox["sdf"].astype(np.float64) - st.sdf).max()) / float(vol.p.m_truncation)
    dc = np.abs(gvox["color"].astype(np.int64) - ovox["color"].astype(np.int64))
    print("organic, %s contract: %d blocks, sdf within %.3g x truncation of the float64 restatement after %d integrations, %d colour bytes differ from the oracle's"
          % (arith, int((gh["ptr"] != FREE_ENTRY).sum()), ds, vc.ORGANIC_INTEGRATIONS, int((dc != 0).sum())))
    if arith == "exact":
        assert np.array_equal(gvox.view(np.uint8), ovox.view(np.uint8))
    else:
        assert ds <= SDF_TOL_LONG and not dc.any()          # integrations only: the colour blend has no ties
    vol.run_batch(vc.organic_ops("de"))
    vol.gs.garbage_collect()
    gh, gheap, gcnt, gvox = vol.gs.download()
    assert vc.is_empty(gh, gheap, gcnt, gvox, vol.p), "%d entries allocated, %d voxels with a byte set" % (
        int((gh["ptr"] != FREE_ENTRY).sum()), int(gvox.view(np.uint8).reshape(len(gvox), -1).any(axis=1).sum()))
