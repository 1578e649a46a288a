"""The numpy model of the placed view-factor calls (tests/placed_vf_model.py) against what it must reduce to and against the analytic
form factor of two opposed plates.  CPU only: the rays are traced by the oracle."""
import numpy as np
import pytest

import placed_vf_model as model
import vf_groups_model as sibling
from helpers import assert_rays_equal, build_oracle
from scene_kit import scenes_module

PLATES_RAYS, PLATES_SEED = 4096, 5
SIGMA = np.sqrt(0.2 * 0.8 / 32768)  # the binomial error of a form factor of 0.2 from 8 x 4096 rays: the margin of the cube test


class Rc:
    """What the scene makers of the model read of the product module: its scene generators (pure numpy)."""
    scenes = scenes_module()


@pytest.fixture(scope="module")
def plates(oracle):
    o = build_oracle(oracle, model.plates_cfg(Rc))
    return o, model.Traced(o, PLATES_RAYS, PLATES_SEED, "cosine")


@pytest.fixture(scope="module")
def mixed(oracle):
    return build_oracle(oracle, model.mixed_cfg(Rc))


@pytest.mark.parametrize("sampling", model.SAMPLINGS)
def test_identity_instance_draws_the_siblings_rays(oracle, sampling):
    sc = Rc.scenes
    verts = np.concatenate([sc.fan_sphere(12, 7, centre=(0.25, 0.5, 0.75), radius=0.5), sc.box_room((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), 2)]).astype(np.float32)
    assert not (np.signbit(verts) & (verts == 0)).any()  # -0 + 0 = +0 under the identity: outside the identity
    o = build_oracle(oracle, {"blas": [(verts, np.arange(1, len(verts) + 1, dtype=np.uint32))], "instances": [(1, sc.IDENTITY3x4[None], np.zeros(1, np.uint32))]})
    prims = o.blas_prims
    assert np.array_equal(model.bases(o), [0, len(prims)])
    assert model.world_triangles(o).tobytes() == prims["v"].tobytes()
    idx = np.arange(3, 203, dtype=np.uint64)
    for q in (0, 1, 77, 143, 144, len(prims) - 1):
        assert_rays_equal(model.placed_rays(o, q, idx, 99, sampling), sibling.sampled_rays(prims, q, idx, 99, sampling), f"placed primitive {q}, {sampling}")


def test_bases_and_world_triangles_of_the_mixed_scene(mixed):
    base = model.bases(mixed)
    assert base.dtype == np.uint32 and np.array_equal(base, np.cumsum([0, 8, 144, 8, 144, 144, 8, 144, 40]))
    tris = model.world_triangles(mixed)
    assert tris.dtype == np.float32 and tris.shape == (640, 3, 3)
    # against float64: the transforms do what they say (a mirror flips the winding's normal, the scaled sphere is an ellipsoid)
    inst, flat = model.placed_index(mixed)
    m = mixed.instances["transform"].astype(np.float64).reshape(-1, 3, 4)[inst]
    v = mixed.blas_prims["v"].astype(np.float64)[flat]
    want = np.einsum("prc,pkc->pkr", m[:, :, :3], v) + m[:, None, :, 3]
    assert np.abs(tris - want).max() < 1e-5
    n_local = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n_world = np.cross(want[:, 1] - want[:, 0], want[:, 2] - want[:, 0])
    mirrored = inst == 2
    assert (n_local[mirrored][:, 2] > 0).all() and (n_world[mirrored][:, 2] < 0).all()  # x -> -x with the vertex order kept: the mirror flips the normal
    assert (np.linalg.det(m[mirrored][:, :, :3]) < 0).all()


def test_the_two_plates(plates):
    o, traced = plates
    assert traced.n == 16 and np.array_equal(model.bases(o), [0, 8, 16])
    groups = np.repeat(np.arange(2, dtype=np.uint32), 8)
    matrix, escaped, uncounted = traced.count(groups, 2)
    total = 8 * PLATES_RAYS
    F = matrix.astype(np.float64) / total
    print("plates: F[0, 1] = %.6f, F[1, 0] = %.6f, analytic %.6f, 4 sigma = %.6f" % (F[0, 1], F[1, 0], sibling.F_OPPOSITE, 4 * SIGMA))
    for a, b in ((0, 1), (1, 0)):
        assert abs(F[a, b] - sibling.F_OPPOSITE) <= 4 * SIGMA, (a, b, F[a, b])
    assert matrix[0, 0] == 0 and matrix[1, 1] == 0 and not uncounted.any()
    assert np.array_equal(matrix.sum(axis=1, dtype=np.uint64) + escaped, np.full(2, total, np.uint64))  # the escapes are the rest of each row, exactly


@pytest.mark.parametrize("sampling", model.SAMPLINGS)
def test_row_sums(mixed, sampling):
    rays, G = 24, 7
    traced = model.Traced(mixed, rays, 13, sampling)
    n = traced.n
    groups = np.repeat(np.arange(8, dtype=np.uint32), np.diff(model.bases(mixed)))  # the room is group 7: excluded under G = 7
    groups[20:30] = model.U32_MAX
    weights = np.random.default_rng(4).integers(0, 1 << 32, n, dtype=np.uint32)
    weights[:3] = (model.U32_MAX, 0, 1 << 31)
    for w in (None, weights):
        for esc in (True, False):
            matrix, escaped, uncounted = traced.count(groups, G, w, esc)
            assert matrix.any() and uncounted.any() and escaped.any() == esc
            ww = np.ones(n, np.uint64) if w is None else w.astype(np.uint64)
            with np.errstate(over="ignore"):
                per_group = np.array([ww[groups == g].sum(dtype=np.uint64) for g in range(G)], dtype=np.uint64) * np.uint64(rays)
                assert np.array_equal(matrix.sum(axis=1, dtype=np.uint64) + escaped + uncounted, per_group)
