"""CPU checks of the diffuse-bounce model (tests/bounce_model.py) that the GPU tests compare rc_bounce_rays_device against: its ports equal
the oracle's primitives, the restated view-factor ray equals the oracle's bit for bit (the pieces the bounce shares with it), and the
sampler has the distribution it claims."""
import ctypes as C

import numpy as np
import pytest

import bounce_model as bm


@pytest.fixture(scope="module")
def L(oracle):
    return bm.oracle_primitives(oracle)


def test_philox_port_equals_oracle(L):
    g = np.random.default_rng(1)
    n = 100_000
    ctr = g.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64)
    ctr[:1000, 1:] = 0  # small counters, as the stages use
    keys = [(0, 0), (0xC4, 0), (0xDEADBEEF, 0x12345678), (0xFFFFFFFF, 0xFFFFFFFF)]
    for k0, k1 in keys:
        got = np.stack(bm.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], k0, k1), axis=1)
        idx = np.concatenate([np.arange(1000), g.choice(n, 2000, replace=False)]) if (k0, k1) != keys[0] else np.arange(n)
        key = (C.c_uint32 * 2)(k0, k1)
        out = (C.c_uint32 * 4)()
        for i in idx:
            c = (C.c_uint32 * 4)(*[int(x) for x in ctr[i]])
            L.rco_philox4x32_10(c, key, out)
            assert tuple(out) == tuple(int(x) for x in got[i]), (i, k0, k1)


def test_sincos_and_acos_ports_equal_oracle(L):
    g = np.random.default_rng(2)
    f32 = np.float32
    theta = np.concatenate([
        g.uniform(-np.pi / 4, 0, 60_000).astype(f32),          # the bounce's negative branch
        g.uniform(0, 3 * np.pi / 4, 30_000).astype(f32),       # its positive range
        g.uniform(0, 2 * np.pi, 20_000).astype(f32),           # view factors' phi
        np.array([-bm.PI_F32 / f32(4), np.nextafter(f32(0), f32(-1)), f32(-0.0), f32(0), bm.PI_F32 / f32(4), bm.PI_F32 / f32(2),
                  f32(3) * bm.PI_F32 / f32(4), f32(2) * bm.PI_F32], f32),
    ]).astype(np.float64)
    s, c = bm.sincos_f64(theta)
    os_, oc = C.c_double(), C.c_double()
    for i, x in enumerate(theta):
        L.rco_sincos_f64(float(x), C.byref(os_), C.byref(oc))
        assert np.float64(os_.value).tobytes() + np.float64(oc.value).tobytes() == s[i].tobytes() + c[i].tobytes(), x
    # on [-pi/4, 0) the reduction is the identity (k = 0): the values are the fdlibm kernels' own, close to libm
    neg = theta < 0
    assert np.all(np.abs(s[neg] - np.sin(theta[neg])) < 1e-15) and np.all(np.abs(c[neg] - np.cos(theta[neg])) < 1e-15)
    x = np.concatenate([g.uniform(0, 1, 20_000).astype(f32), np.array([0, 0.5, np.nextafter(f32(0.5), f32(0)), np.nextafter(f32(1), f32(0))], f32)])
    x = np.minimum(x, np.nextafter(f32(1), f32(0))).astype(np.float64)  # acos' domain here is [0, 1), as u32_to_unit's
    a = bm.acos_f64(x)
    for i, xi in enumerate(x):
        assert L.rco_acos_f64(float(xi)) == a[i], xi


def test_view_factor_ray_restated_bit_exact(oracle):
    """Scene.view_factor_ray (the oracle's restatement of view_factors!' sampler) equals the model's: Philox keying, u32_to_unit,
    get_orthogonal_basis and sincos_f64 are the same pieces the bounce uses."""
    import raycore_jl_amd as rc
    s = oracle.Scene()
    s.add_blas(rc.scenes.random_triangles(64, 0xB0))
    s.add_blas(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1, 1, 0, 0], [1, 1, 1, 2, 1, 1, 1, 2, 1]], np.float32))  # axis normals
    s.add_instance(1)
    s.add_instance(2)
    s.build()
    prims = s.blas_prims
    for seed in (0, 0xC4, 0x1234_5678_9ABC_DEF0):
        for src in range(len(prims)):
            got = bm.view_factor_ray(prims, src, np.arange(40), seed)
            want = np.array([s.view_factor_ray(src, i, seed) for i in range(40)])
            assert got.tobytes() == want.tobytes(), (seed, src)


NORMALS = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0),           # axis-aligned
           (1, 1, 0), (0, 1, 1), (1, 1, 1), (-1, 1, -1),           # min_abs_coord ties
           (0.3, -0.5, 0.81), (-0.9, 0.1, 0.2)]


def test_sampler_distribution():
    n_per = 100_000
    f32 = np.float32
    zs, cos = [], []
    for j, nv in enumerate(NORMALS):
        nn = np.asarray(nv, f32)
        nn = nn / np.sqrt(np.dot(nn, nn)).astype(f32)
        nrm = np.broadcast_to(nn.astype(f32), (n_per, 3))
        u1, u2 = bm.bounce_uniforms(np.arange(j * n_per, (j + 1) * n_per), 0, 0, 0xC4)
        d, z = bm.cosine_hemisphere(nrm, u1, u2)
        ct = d.astype(np.float64) @ nn.astype(np.float64)
        # closed hemisphere: z >= 0 exactly; in world space up to the basis' rounding (u, v are orthogonal to n within a few ulps)
        assert np.all(z >= 0) and np.all(ct >= -4e-7), nv
        assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) <= 1e-6), nv
        zs.append(z.astype(np.float64))
        cos.append(ct)
        assert abs(ct.mean() - 2 / 3) < 4 * np.sqrt(1 / 18 / n_per), nv  # E[cos] = 2/3, Var = 1/2 - 4/9
    z2 = np.concatenate(zs) ** 2
    assert len(z2) >= 10 ** 6
    counts, _ = np.histogram(z2, bins=50, range=(0, 1))  # cos^2 is uniform on [0, 1] for a cosine-weighted hemisphere
    expect = len(z2) / 50
    chi2 = ((counts - expect) ** 2 / expect).sum()
    assert chi2 < 100, chi2  # 49 dof: p ~ 3e-5
    assert abs(np.concatenate(cos).mean() - 2 / 3) < 1e-3


def test_model_dead_slots_and_sources():
    s, k, live = bm.sources(7, np.array([4, 2, 9], np.uint32), 3, wrap=True)
    assert s.tolist() == [4, 2, 9, 4, 2, 9, 4] and k.tolist() == [0, 0, 0, 1, 1, 1, 2] and live.all()
    s, k, live = bm.sources(5, np.array([4, 2, 9], np.uint32), 2, wrap=False)
    assert live.tolist() == [True, True, False, False, False] and s[:2].tolist() == [4, 2]
    assert not bm.sources(5, np.array([4], np.uint32), 0, wrap=True)[2].any()
