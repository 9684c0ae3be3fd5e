"""The first-hit emission layer without a GPU: the symbols and Python names exist, the ABI version stands, split and merge
refuse bad arguments before any device work, and the float32 model of tests/_emission_model.py agrees with hand-made buffers and has
the property the split exists for: a pixel an emitter partly covers demodulates to the illumination of what lies beside the emitter."""
import os
import re

import numpy as np
import pytest

import _emission_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbrhip_render_features_emission", "pbrhip_render_features_emission_device", "pbrhip_emission_split", "pbrhip_emission_split_device",
           "pbrhip_emission_merge", "pbrhip_emission_merge_device")
EINVAL, ENODEVICE = -1, -3
F = np.float32
EPS = float(np.finfo(F).eps)


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("EmissionLayer", "RenderFeaturesEmission", "SplitEmission", "MergeEmission"):
        assert hasattr(api, name) and hasattr(pa, name), name
    assert L.pbrhip_abi_version() == 6 and re.search(r"#define PBRHIP_ABI_VERSION 6u\b", hdr)  # functions only: the layouts stand
    shim = open(os.path.join(ROOT, "include", "pbrlab_hip.hpp")).read()
    for name in ("EmissionLayer", "RenderFeaturesEmission", "SplitEmission", "MergeEmission"):
        assert re.search(r"\b" + name + r"\b", shim), name


def _refused(fs, args, word=b""):
    from pbrlab_amd import _lib
    L = _lib.lib()
    for f in fs:
        rc = f(*args)
        assert rc == EINVAL and word in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())


def test_split_and_merge_refuse_bad_arguments_before_any_device_work():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib
    L = _lib.lib()
    W, H = 8, 4
    img = [np.zeros((H, W, 4), F) for _ in range(5)]
    rgba, em, alb, out, oalb = (a.ctypes.data for a in img)
    one = [np.ones((H, W), np.uint32) for _ in range(2)]
    count, fc = (a.ctypes.data for a in one)
    fs = (L.pbrhip_emission_split, L.pbrhip_emission_split_device)
    #       0  1  2  3     4      5   6    7   8    9
    good = [0, W, H, rgba, count, em, alb, fc, out, oalb]

    def swap(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    _refused(fs, swap(_1=0), b"empty")
    _refused(fs, swap(_2=0), b"empty")
    for k in (3, 4, 5, 8):  # NULL rgba, count, emission, out_rgba
        _refused(fs, swap(**{f"_{k}": None}), b"NULL")
    for k in (6, 7, 9):  # one of the albedo triple missing
        _refused(fs, swap(**{f"_{k}": None}), b"together")
    for a, b in ((6, 7), (6, 9), (7, 9)):  # two missing
        _refused(fs, swap(**{f"_{a}": None, f"_{b}": None}), b"together")
    for k in (3, 4, 5, 7):  # out_albedo_hits is rgba, count, emission, feature_count
        _refused(fs, swap(_9=good[k]), b"out_albedo_hits is an input")
    fm = (L.pbrhip_emission_merge, L.pbrhip_emission_merge_device)
    #        0  1  2  3     4   5      6
    goodm = [0, W, H, rgba, em, count, out]
    _refused(fm, goodm[:1] + [0] + goodm[2:], b"empty")
    _refused(fm, goodm[:2] + [0] + goodm[3:], b"empty")
    for k in (3, 4, 5, 6):
        _refused(fm, goodm[:k] + [None] + goodm[k + 1:], b"NULL")
    # what is allowed gets as far as the device (none here: ENODEVICE; one there: 0): the in-place forms and no albedo triple
    want = 0 if pa.device_count() > 0 else ENODEVICE
    assert L.pbrhip_emission_split(*good) == want
    assert L.pbrhip_emission_split(*swap(_8=rgba, _9=alb)) == want
    assert L.pbrhip_emission_split(*swap(_6=None, _7=None, _9=None)) == want
    assert L.pbrhip_emission_merge(*goodm) == want
    assert L.pbrhip_emission_merge(*goodm[:6], rgba) == want
    # the feature pass: the NULL checks of pbrhip_render_features
    for f in (L.pbrhip_render_features_emission, L.pbrhip_render_features_emission_device):
        assert f(None, None, None, None, None, None) == EINVAL and b"NULL" in L.pbrhip_last_error()


def test_python_refuses_mixed_and_misshapen_buffers():
    import pbrlab_amd as pa
    layer = pa.RenderLayer(8, 4)
    with pytest.raises(ValueError):
        pa.SplitEmission(layer, np.zeros((4, 9, 4), F))
    with pytest.raises(ValueError):
        pa.SplitEmission(layer, pa.EmissionLayer(8, 4), pa.FeatureLayer(8, 5))
    with pytest.raises(ValueError):
        pa.MergeEmission(np.zeros((4, 8, 4), F), pa.EmissionLayer(8, 4), np.zeros((4, 7), np.uint32))
    if pa.device_count() == 0:
        with pytest.raises(pa.PbrHipError) as e:
            pa.SplitEmission(layer, pa.EmissionLayer(8, 4))
        assert e.value.code == ENODEVICE
        with pytest.raises(pa.PbrHipError) as e:
            pa.MergeEmission(np.zeros((4, 8, 4), F), pa.EmissionLayer(8, 4), layer.count)
        assert e.value.code == ENODEVICE


def test_model_on_hand_made_buffers():
    #                 plain            emission only    more emission than colour (clamped)  no samples        NaN difference
    rgba = np.array([[[3.0, 2.0, 1.0, 4], [8.0, 8.0, 8.0, 2], [1.0, 5.0, 0.25, 2], [9.0, 9.0, 9.0, 7], [np.inf, 1.0, 1.0, 1]]], F)
    em = np.array([[[1.0, 0.5, 0.0, 1], [8.0, 8.0, 8.0, 2], [2.0, 1.0, 0.25, 1], [1.0, 1.0, 1.0, 1], [np.inf, 0.5, 0.0, 1]]], F)
    count = np.array([[4, 2, 2, 0, 1]], np.uint32)
    alb = np.array([[[1.5, 1.0, 0.5, 3], [0, 0, 0, 2], [0.5, 0.5, 0.5, 1], [0, 0, 0, 0], [0.25, 0.25, 0.25, 1]]], F)
    fc = np.array([[4, 2, 2, 0, 1]], np.uint32)
    out, oalb = EM.split(rgba, count, em, alb, fc)
    assert out.dtype == F and oalb.dtype == F
    assert out.tolist() == [[[2.0, 1.5, 1.0, 4.0], [0.0, 0.0, 0.0, 2.0], [0.0, 4.0, 0.0, 2.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.5, 1.0, 1.0]]]
    assert oalb.tolist() == [[[1.5, 1.0, 0.5, 4.0], [0, 0, 0, 2.0], [0.5, 0.5, 0.5, 2.0], [0, 0, 0, 0.0], [0.25, 0.25, 0.25, 1.0]]]
    assert not np.signbit(out).any()  # (a zero is +0)
    assert EM.split(rgba, count, em)[1] is None and np.array_equal(EM.split(rgba, count, em)[0], out)
    # with hits := samples the albedo the filters divide by is albedo.rgb / samples: a miss is black
    assert np.array_equal(EM.clamped_albedo(oalb, fc)[0, 0], np.array([1.5, 1.0, 0.5], F) / F(4))
    assert np.array_equal(EM.clamped_albedo(alb, fc)[0, 0], (np.array([1.5, 1.0, 0.5], F) + F(1)) / F(4))
    assert np.array_equal(EM.clamped_albedo(oalb, fc)[0, 1], np.full(3, 1e-3, F)) and np.array_equal(EM.clamped_albedo(oalb, fc)[0, 3], np.ones(3, F))
    filtered = np.array([[[0.5, 0.25, 0.125, 1], [0, 0, 0, 1], [1, 1, 1, 0.5], [0.75, 0.5, 0.25, 0], [2, 2, 2, 1]]], F)
    em[0, 4] = (3.0, 1.0, 0.0, 1)
    got = EM.merge(filtered, em, count)
    assert got.dtype == F
    assert got.tolist() == [[[0.75, 0.375, 0.125, 1.0], [4.0, 4.0, 4.0, 1.0], [2.0, 1.5, 1.125, 0.5], [0.75, 0.5, 0.25, 0.0], [5.0, 3.0, 2.0, 1.0]]]
    # one rounding per operation: a third is not exact
    third = EM.merge(np.zeros((1, 1, 4), F), np.array([[[1.0, 2.0, 0.1, 3]]], F), np.array([[3]], np.uint32))
    assert np.array_equal(third[0, 0, :3], np.array([F(1.0) / F(3.0), F(2.0) / F(3.0), F(0.1) / F(3.0)], F))


@pytest.mark.parametrize("Le, a_lo, e_lo", [(2.0, 0.5, 1.0), (17.0, 0.05, 0.2)])
def test_model_split_removes_the_coverage_from_the_demodulated_illumination(Le, a_lo, e_lo):
    """A pixel whose four samples see an emitter (radiance Le, black albedo) k times and a surface of albedo a_c under illumination e_c
    otherwise: colour sum S = k Le + (4 - k) a_c e_c, albedo sum (4 - k) a_c.  Plain demodulation ((S / 4) / a with a = albedo sum / 4)
    depends on k; after the split ((S - E) / 4) / a' = e_c for every k < 4, and exactly 0 for k = 4.

    The bound: S and E are float32 sums of four terms in sample order, so S - E differs from the reflected sum R = (4 - k) a_c e_c by at
    most the roundings of S's three additions, 3 (eps / 2) S, and of E's (the same bound; E <= S); the subtraction is one more rounding
    and the two divisions and the albedo's product and division one each: |e - e_c| / e_c <= eps (3 S / R + 3).  With an emitter about as
    bright as the surface (Le <= 2, a_c e_c >= 0.5: S / R <= 13) that is a few ulp, at most 42; with the Cornell box's 17 beside a dark
    surface it is the cancellation S - E pays, still orders of magnitude below the jump it removes."""
    rng = np.random.RandomState(18)
    worst = 0.0
    for trial in range(200):
        a_c = rng.uniform(a_lo, 0.9, 3).astype(F)
        e_c = rng.uniform(e_lo, 3.0, 3).astype(F)
        le = (F(Le) * rng.uniform(0.5, 1.0, 3)).astype(F)
        refl = a_c * e_c  # one sample's reflected radiance (float32, exact for the model: the renderer's own product)
        plain = []
        for k in range(5):
            seen = np.zeros(4, bool)
            seen[rng.permutation(4)[:k]] = True
            S, E, A = np.zeros(3, F), np.zeros(3, F), np.zeros(3, F)
            for i in range(4):  # ascending pass order, one rounding per addition
                S = S + (le if seen[i] else refl)
                if seen[i]:
                    E = E + le
                else:
                    A = A + a_c
            rgba = np.array([[[*S, 4]]], F)
            em = np.array([[[*E, k]]], F)
            alb = np.array([[[*A, 4]]], F)  # (the emitter is a hit, of black albedo)
            cnt = np.array([[4]], np.uint32)
            out, oalb = EM.split(rgba, cnt, em, alb, cnt)
            e = (out[0, 0, :3] / F(4)) / EM.clamped_albedo(oalb, cnt)[0, 0]
            plain.append((S / F(4)) / EM.clamped_albedo(alb, cnt)[0, 0])
            if k == 4:
                assert (e == 0).all() and (out[0, 0, :3] == 0).all()
                continue
            R = (4 - k) * refl.astype(np.float64)
            rel = np.abs(e.astype(np.float64) - refl.astype(np.float64) / a_c.astype(np.float64)) / (refl.astype(np.float64) / a_c.astype(np.float64))
            bound = EPS * (3.0 * S.astype(np.float64) / R + 3.0)
            assert (rel <= bound).all(), (k, rel, bound)
            if k == 0:
                assert (rel <= 4 * EPS).all()
            worst = max(worst, float((rel / EPS).max()))
        # what the split removes: the plain quotient moves with k by far more than the bound
        assert np.max(np.abs(plain[3] - plain[0]) / plain[0]) > 0.1
    print(f"Le = {Le}: worst |e - e_c| / e_c = {worst:.1f} eps")
    assert worst <= 3.0 * (3.0 * Le / (a_lo * e_lo) + 1.0) + 3.0  # (the bound at k = 3 and the dimmest surface: 42 eps for the first case)


def test_cli_refuses_split_emission_without_a_consumer():
    import subprocess
    from pbrlab_amd import io_api
    for args in (["--split-emission"], ["--split-emission", "--denoise", "--adaptive", "0.1"]):
        r = subprocess.run([io_api.CLI_PATH, "scene.obj"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--split-emission needs --aov or --denoise" in r.stderr, (args, r.returncode, r.stderr)
