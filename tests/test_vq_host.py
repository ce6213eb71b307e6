"""Host (no GPU): the quantiser's surface (include/fishvoc.h fv_vq_*, vocoder_amd/modules/quantizers.py) — the restatement's score form
against encodec's literal distance, the buffer names a VQVAEModel checkpoint carries, the refusals that name their field, and
UnifyGenerator without a quantiser."""
import ctypes

import numpy as np
import pytest
import torch

import vq_reference as vref
from vocoder_amd import _lib
from vocoder_amd.modules.quantizers import ResidualVectorQuantization, VectorQuantization, VQResult

ENCODEC_BUFFERS = ["_codebook.inited", "_codebook.cluster_size", "_codebook.embed", "_codebook.embed_avg"]


@pytest.mark.parametrize("D,K", [(64, 256), (7, 5), (96, 320)])
def test_score_form_picks_the_codes_of_the_literal_distance(D, K):
    x, (embed,) = vref.make_case(D, K, 1, 200, seed=3)
    codes, gap, tau = vref.search(x, embed)
    lit = vref.literal_codes(x, embed)
    dec = gap > tau
    assert dec.mean() >= 0.99
    # h is rounded to fp32 in the score form: the two can differ only where the gap is inside that rounding, far inside tau
    assert np.array_equal(codes[dec], lit[dec])


def test_reference_edge_cases():
    embed = np.array([[1, 0], [1, 0], [0, 1]], np.float32)
    x = np.array([[2, 0], [np.nan, np.nan], [0, 3]], np.float32)
    codes, z, dec = vref.encode(x, [embed])
    assert codes.tolist() == [[0, 0, 2]] and not dec[0] and not dec[1] and dec[2]
    assert np.array_equal(z[0], embed[0]) and np.array_equal(z[2], embed[2])
    assert np.array_equal(vref.gather_sum(np.array([[-1, 2]]), [embed]), np.array([[0, 0], [0, 1]], np.float32))


def test_buffer_names_are_encodecs_and_round_trip_strictly():
    vq = VectorQuantization(dim=8, codebook_size=16, kmeans_init=False)
    assert list(vq.state_dict()) == ENCODEC_BUFFERS
    assert vq.state_dict()["_codebook.embed"].shape == (16, 8) and vq.state_dict()["_codebook.inited"].tolist() == [1.0]
    rvq = ResidualVectorQuantization(dim=8, codebook_size=16, num_quantizers=3, kmeans_init=False)
    assert list(rvq.state_dict()) == [f"layers.{i}.{k}" for i in range(3) for k in ENCODEC_BUFFERS]
    for m, make in ((vq, lambda: VectorQuantization(8, 16)), (rvq, lambda: ResidualVectorQuantization(num_quantizers=3, dim=8, codebook_size=16))):
        other = make()
        res = other.load_state_dict(m.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        for k, v in m.state_dict().items():
            assert torch.equal(other.state_dict()[k], v)
    with pytest.raises(RuntimeError):
        vq.load_state_dict({**vq.state_dict(), "project_in.weight": torch.zeros(8, 8)}, strict=True)
    z, codes, loss = VQResult(1, 2, 3)        # unpacks as encodec's tuple, serves unify.py's attributes
    assert (z, codes, loss) == (1, 2, 3) and VQResult(1, 2, 3).z == 1 and VQResult(1, 2, 3).codes == 2


def test_python_refusals_name_the_field():
    with pytest.raises(ValueError, match="codebook_dim"):
        VectorQuantization(dim=8, codebook_size=16, codebook_dim=4)
    VectorQuantization(dim=8, codebook_size=16, codebook_dim=8)
    with pytest.raises(ValueError, match="dim"):
        VectorQuantization(dim=0, codebook_size=16)
    with pytest.raises(ValueError, match="codebook_size"):
        VectorQuantization(dim=8, codebook_size=65537)
    with pytest.raises(ValueError, match="num_quantizers"):
        ResidualVectorQuantization(num_quantizers=33, dim=8, codebook_size=16)
    vq = VectorQuantization(dim=8, codebook_size=16).eval()
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        vq(torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="inference-only"):
        vq.train()(torch.zeros(1, 8, 3))


@pytest.mark.parametrize("cfg,field", [((0, 16, 1), "dim"), ((4097, 16, 1), "dim"), ((8, 65537, 1), "codebook_size"), ((8, 0, 1), "codebook_size"),
                                       ((8, 16, 33), "num_quantizers"), ((8, 16, 0), "num_quantizers")])
def test_create_refuses_and_names_the_field(cfg, field):
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.fv_vq_create(ctypes.byref(_lib.VQConfig(*cfg)), ctypes.byref(h)) == _lib.FV_ERR_INVALID
    assert not h.value and L.fv_last_error().decode().startswith(f"fv_vq_create: {field} =")


def test_create_and_shape_validation_without_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.fv_vq_create(ctypes.byref(_lib.VQConfig(512, 4096, 8)), ctypes.byref(h)) == _lib.FV_OK and h.value
    try:
        assert L.fv_vq_workspace_bytes(h, -1, 4) == 0 and "batch" in L.fv_last_error().decode()
        assert L.fv_vq_workspace_bytes(h, 2, -4) == 0 and "T =" in L.fv_last_error().decode()
        assert L.fv_vq_workspace_bytes(h, 65535, 1 << 20) == 0 and "T =" in L.fv_last_error().decode()
        assert L.fv_vq_workspace_bytes(h, 0, 4) == 0
        assert L.fv_vq_load_codebook(h, 8, (ctypes.c_float * 4)()) == _lib.FV_ERR_INVALID and "layer" in L.fv_last_error().decode()
        assert L.fv_vq_set_slices(h, -1) == _lib.FV_ERR_INVALID and "slices" in L.fv_last_error().decode()
        # an encode before the codebooks are in: refused, by layer
        assert L.fv_vq_encode(h, None, 4, None, None, None, 1, 4, None, 0, None) == _lib.FV_ERR_STATE and "layer 0" in L.fv_last_error().decode()
    finally:
        L.fv_vq_destroy(h)


def test_unify_generator_without_a_quantiser_is_unchanged():
    from vocoder_amd.modules.generators import UnifyGenerator
    u = UnifyGenerator(torch.nn.Identity(), torch.nn.Identity())
    assert u.vq is None
    with pytest.raises(ValueError, match="VQ module is not present"):
        u.encode(torch.zeros(1, 2, 3))
    with pytest.raises(ValueError, match="VQ module is not present"):
        u.decode(torch.zeros(1, 3, dtype=torch.int64))
    vq = VectorQuantization(dim=8, codebook_size=16)
    assert UnifyGenerator(torch.nn.Identity(), torch.nn.Identity(), vq=vq).vq is vq
