"""CPU checks of the wider envelope of CARCA.recommend / rank_items (allow_composed=True): the
routing decision of catalogue.carca_route (fused, composed or an error) over a grid of (d, heads, L, decoder,
allow_composed), the keyword's presence on every call that takes it, and the constants the header and _lib share."""
import inspect
import os
import re

import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, long_profile, ops, train
from carca_replication_amd.modules import CARCA, KNN
from tests.model_util import build_model

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
    for fn in (CARCA.recommend, CARCA.rank_items, CARCA.score_items, CARCA.recommend_from, CARCA.score_items_at,
               CARCA.best_context, CARCA.recommend_at, CARCA.recommend_by_group, CARCA.recommend_capped,
               CARCA.recommend_users, CARCA.explain_items, CARCA.explain_top_slots, CARCA.recommend_explained,
               CARCA.recommend_diverse, catalogue.carca_model_side):
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


def test_shared_call_hands_the_keyword_to_the_model_side_only_when_set(monkeypatch):
    class Reached(Exception):
        pass

    seen = []

    def recording(real):  # the arguments the model side was reached with, bound to its real signature; nothing launches
        def stub(*a, **kw):
            seen.append(dict(inspect.signature(real).bind(*a, **kw).arguments))
            raise Reached
        return stub

    monkeypatch.setattr(catalogue, "carca_model_side", recording(catalogue.carca_model_side))
    monkeypatch.setattr(catalogue, "knn_model_side", recording(catalogue.knn_model_side))
    prof = (torch.ones(2, 8, dtype=torch.int64), None, torch.zeros(2, 8, 6))
    ctx = torch.zeros(2, 6)
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="all", decoder="ca"), 50, 24, 6, 12, 8).eval()
    with pytest.raises(Reached):
        model.recommend(prof, ctx, allow_composed=True)
    assert seen[0]["allow_composed"] is True and seen[0]["model"] is model and seen[0]["what"] == "recommend"
    with pytest.raises(Reached):
        model.recommend(prof, ctx)
    assert seen[1].get("allow_composed", False) is False
    knn = KNN()
    with pytest.raises(Reached):  # (a keyword the baseline's model side does not take would fail the bind)
        knn.recommend(prof)
    assert "allow_composed" not in seen[2] and seen[2]["model"] is knn and len(seen) == 3


def test_constants_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "carca_hip.h")) as f:
        text = f.read()
    defs = dict(re.findall(r"#define (CARCA_MAX_L|CARCA_MAX_PROFILE_L) (\d+)", text))
    assert int(defs["CARCA_MAX_L"]) == _lib.MAX_L == 64
    assert int(defs["CARCA_MAX_PROFILE_L"]) == _lib.MAX_PROFILE_L == 1024


def test_forward_and_the_catalogue_calls_share_one_encoder():
    assert "encode(model" in inspect.getsource(long_profile.forward)
    assert "long_profile.encode(model" in inspect.getsource(catalogue._carca_context_free)
    assert "sa_block(" not in inspect.getsource(long_profile.forward)  # (the block loop lives in encode alone)
