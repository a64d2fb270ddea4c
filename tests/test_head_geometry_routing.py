"""CPU checks of the head-geometry routing: which (d, H) the fused attention kernels are built for
(carca_attn_geometry_built, against the DESIGN.md section 1 table restated here from carca_padded_dims' rule), and that
ops.use_composed -- the one rule CARCA.forward, forward_nograd and the two stand-alone blocks route on -- sends every
other model to the composed path instead of to a "no kernel built" error."""
import pytest
import torch

# the (DPI, DHP, H) the fused kernels are instantiated for
BUILT = {(64, 16, 4), (64, 32, 2), (64, 64, 1), (96, 32, 3), (96, 48, 2), (96, 96, 1), (128, 32, 4), (128, 64, 2),
         (128, 128, 1)}


def _pairs(d_max=128):
    return [(d, H) for d in range(1, d_max + 1) for H in range(1, d + 1) if d % H == 0]


def _geometry(d, H):
    dpi = 64 if d <= 64 else (96 if d <= 96 else 128)
    return dpi, (d // H + 15) // 16 * 16, H


def test_geometry_built_matches_the_design_table_for_every_pair():
    from carca_replication_amd import _lib, ops

    lib = _lib.load()
    pairs = _pairs()
    assert len(pairs) == 645
    built = [(d, H) for d, H in pairs if _geometry(d, H) in BUILT]
    assert len(built) == 131
    for d, H in pairs:
        want = _geometry(d, H) in BUILT
        assert lib.carca_attn_geometry_built(d, H) == int(want), (d, H)
        assert ops.attn_geometry_built(d, H) is want, (d, H)
        dpi, dhp, dpo = ops.padded_dims(d, H)
        assert (dpi, dhp, H) == _geometry(d, H) and dpo == H * dhp
    # every built geometry is reached by some (d, H)
    assert {_geometry(d, H) for d, H in built} == BUILT


def test_geometry_built_never_errors_outside_the_envelope():
    from carca_replication_amd import _lib

    lib = _lib.load()
    for d, H in [(129, 1), (256, 2), (256, 4), (1024, 8), (90, 4), (7, 2)]:
        assert lib.carca_attn_geometry_built(d, H) == 0, (d, H)


def test_use_composed_is_exactly_unbuilt_or_too_wide_or_too_long():
    from carca_replication_amd import _lib, ops

    for d, H in _pairs(256):
        built = d <= 128 and _geometry(d, H) in BUILT
        for L in (1, 50, _lib.MAX_L):
            assert ops.use_composed(d, [H], L) is (not built), (d, H, L)
            assert ops.use_composed(d, [H, H], L, n_groups=_lib.MAX_GROUPS) is (not built), (d, H, L)
        assert ops.use_composed(d, [H], _lib.MAX_L + 1)
        assert ops.use_composed(d, [H], 20, n_groups=_lib.MAX_GROUPS + 1)
    # a model is fused only if EVERY attention module's geometry is built; no attention module at all: nothing to check
    assert ops.use_composed(90, [3, 3], 50) is False
    assert ops.use_composed(64, [2, 8], 50) is True
    assert ops.use_composed(48, [], 50) is False


@pytest.mark.parametrize("d,H", [(96, 4), (32, 2), (64, 8), (128, 8), (48, 1), (80, 4), (60, 3)])
def test_unbuilt_configurations_route_composed_in_every_module(d, H):
    """The modules decide through ops.use_composed (no GPU needed: the decision precedes any launch)."""
    from carca_replication_amd import ops
    from tests.model_util import build_model

    assert not ops.attn_geometry_built(d, H)
    model = build_model(dict(d=d, H=H, n_blocks=2), 300, 16, 2, 5, 20)
    assert model._attn_heads() == [H, H, H]
    assert model._composed((torch.zeros(2, 20, dtype=torch.int32),), [None, None])
    assert ops.use_composed(d, [model.encoder[0].attn.H], 20)
    assert ops.use_composed(d, [model.decoder.attn.H], 20)
