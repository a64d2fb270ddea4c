"""CPU checks of the wider envelope of CARCA.recommend / rank_items (allow_composed=True): the
routing decision of catalogue.carca_route (fused, composed or an error) over a grid of (d, heads, L, decoder,
allow_composed), the keyword's presence on every call that takes it, and the constants the header and _lib share."""
import inspect
import os
import re

import pytest

from carca_replication_amd import CarcaHipError, _lib, catalogue, long_profile, ops, train
from carca_replication_amd.modules import CARCA, KNN

# (d, H) with a fused attention geometry built (CARCA_ATT_GEOMETRIES), and without one
BUILT = [(64, 4), (62, 2), (64, 1), (90, 3), (96, 2), (90, 1), (128, 4), (120, 2), (128, 1)]
UNBUILT = [(100, 5), (48, 1), (64, 8), (96, 4)]


def test_geometry_lists_are_what_the_library_says():
    for d, H in BUILT:
        assert ops.attn_geometry_built(d, H), (d, H)
    for d, H in UNBUILT:
        assert not ops.attn_geometry_built(d, H), (d, H)


def _route(d, enc, L, dec, allow):
    return catalogue.carca_route("recommend", d, enc, L, dec, allow)


@pytest.mark.parametrize("L", [1, 50, 64])
@pytest.mark.parametrize("dH", BUILT)
def test_inside_the_fused_envelope_the_keyword_changes_nothing(dH, L):
    d, H = dH
    for dec in (None, H):  # a dot decoder, a cross-attention decoder
        for allow in (False, True):
            assert _route(d, [H, H], L, dec, allow) == "fused"
    assert _route(d, [], L, H, True) == "fused"  # no encoder block: nothing to compose below 65 slots


@pytest.mark.parametrize("L", [65, 100, 1024])
@pytest.mark.parametrize("dH", BUILT)
def test_long_profiles(dH, L):
    d, H = dH
    for dec in (None, H):
        with pytest.raises(CarcaHipError, match="64") as e:
            _route(d, [H], L, dec, False)
        assert "allow_composed" in str(e.value)
        assert _route(d, [H], L, dec, True) == "composed"
        with pytest.raises(CarcaHipError, match="1024"):
            _route(d, [H], 1025, dec, True)


@pytest.mark.parametrize("L", [20, 64, 65])
@pytest.mark.parametrize("dH", UNBUILT)
def test_unbuilt_geometries(dH, L):
    d, H = dH
    # without the keyword: today's error, whichever module has the geometry
    for enc, dec in (([H], None), ([H], H), ([], H)):
        with pytest.raises(CarcaHipError, match=rf"\({d}, {H}\)" if L <= 64 else "64"):
            _route(d, enc, L, dec, False)
    # with it: an unbuilt ENCODER geometry runs composed under a dot decoder ...
    assert _route(d, [H], L, None, True) == "composed"
    # ... a cross-attention decoder still needs its own geometry for the sweep
    with pytest.raises(CarcaHipError, match=rf"\({d}, {H}\)"):
        _route(d, [H], L, H, True)
    built_H = next(h for (dd, h) in BUILT + [(48, 2), (100, 4)] if dd == d and ops.attn_geometry_built(dd, h))
    with pytest.raises(CarcaHipError, match=rf"\({d}, {H}\)"):
        _route(d, [built_H], L, H, True)
    assert _route(d, [H], L, built_H, True) == "composed"  # built decoder over an unbuilt encoder
    assert _route(d, [built_H, H], L, None, True) == "composed"  # one unbuilt block is enough


@pytest.mark.parametrize("allow", [False, True])
@pytest.mark.parametrize("L", [16, 100])
def test_wider_than_128_stays_out(allow, L):
    for dec in (None, 2):
        with pytest.raises(CarcaHipError, match="256|64"):
            _route(256, [2], L, dec, allow)
    with pytest.raises(CarcaHipError, match="128"):
        _route(256, [2], 16, None, True)


def test_keyword_is_on_every_call_that_takes_it_and_off_by_default():
    for fn in (CARCA.recommend, CARCA.rank_items, catalogue.recommend, catalogue.rank_items, catalogue.carca_model_side):
        p = inspect.signature(fn).parameters
        assert "allow_composed" in p and p["allow_composed"].default is False, fn
    for fn in (KNN.recommend, KNN.rank_items, catalogue.knn_model_side):
        assert "allow_composed" not in inspect.signature(fn).parameters


def test_evaluate_full_passes_the_keyword_only_to_models_that_take_it():
    class Wide:
        def recommend(self, profile, context, k=10, exclude="profile", candidates=None, allow_composed=False):
            pass

        rank_items = recommend

    class Narrow:
        def recommend(self, profile, context, k=10, exclude="profile"):
            pass

        rank_items = recommend

    for method in ("recommend", "rank_items"):
        assert train._wide_envelope(Wide(), method) == {"allow_composed": True}
        assert train._wide_envelope(Narrow(), method) == {}
    assert train._wide_envelope(KNN.__new__(KNN), "recommend") == {}
    assert train._wide_envelope(CARCA.__new__(CARCA), "rank_items") == {"allow_composed": True}


def test_shared_call_hands_the_keyword_to_the_model_side_only_when_set():
    seen = []

    def fill(what, D, **kw):
        seen.append(kw)
        return [], None

    assert catalogue._fill(fill, "x", None, False) == ([], None) and seen == [{}]
    catalogue._fill(fill, "x", None, True)
    assert seen[1] == {"allow_composed": True}


def test_constants_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "carca_hip.h")) as f:
        text = f.read()
    defs = dict(re.findall(r"#define (CARCA_MAX_L|CARCA_MAX_PROFILE_L) (\d+)", text))
    assert int(defs["CARCA_MAX_L"]) == _lib.MAX_L == 64
    assert int(defs["CARCA_MAX_PROFILE_L"]) == _lib.MAX_PROFILE_L == 1024


def test_forward_and_the_catalogue_calls_share_one_encoder():
    assert "encode(model" in inspect.getsource(long_profile.forward)
    assert "long_profile.encode(model" in inspect.getsource(catalogue.carca_model_side)
    assert "sa_block(" not in inspect.getsource(long_profile.forward)  # (the block loop lives in encode alone)
