"""Scenes built once per test module in the product and in the oracle.  A test file subclasses a world for its own degeneracy guards and
memos and wraps the generators below in a module-scoped fixture of its own: no world is shared between modules (tests set options on
their scenes)."""
import numpy as np

from gpu_kit import dev
from helpers import build_oracle, build_product
from scene_kit import room_cfg


class C3World:
    """C3 with 16 x 9 fan spheres on `lattice`, its 320 x 200 primary rays less three, and the oracle's hits of them."""
    N_RAYS = 63_997

    def __init__(self, rc, oracle, lattice, kernel=None):
        self.cfg = rc.scenes.config_c3(lon=16, bands=9, lattice=lattice)
        self.t, self.o = build_product(rc, self.cfg), build_oracle(oracle, self.cfg)
        if kernel is not None:
            self.t.set_option("kernel", kernel)
        self.rays = rc.scenes.c3_primary_rays(self.cfg, 320, 200)[:self.N_RAYS]
        self.hits = self.o.trace(self.rays, nthreads=16)
        self.lit = self.hits["hit"] == 1
        # a degenerate input cannot pass: enough hits and misses (each test's World adds its own guards)
        lit, missed = int(self.lit.sum()), int((~self.lit).sum())
        assert lit >= 1000 and missed >= 1000, (lit, missed)
        self.d_rays, self.d_hits = dev(self.rays), dev(self.hits)


def three_shapes(World, rc, oracle):
    """The three kernel shapes the launcher dispatches, as {"lds", "partial", "plain"}: World; freed when the generator is resumed."""
    w = {"lds": World(rc, oracle, (3, 3, 2)),            # 18 instances: the whole top level in LDS
         "partial": World(rc, oracle, (7, 7, 6)),        # 294 instances: only the top of the TLAS is staged
         "plain": World(rc, oracle, (3, 3, 2), kernel=3)}  # the small scene again through the 256-thread kernel
    assert w["lds"].t.n_instances() == 18 and w["partial"].t.n_instances() == 294
    yield w
    for x in w.values():
        x.t.free()


class VfWorld:
    """One scene in the product and in the oracle; the oracle's matrices are computed once per (rays, seed) and are read-only."""

    def __init__(self, rc, oracle, cfg):
        self.rc, self.t, self.o = rc, build_product(rc, cfg), build_oracle(oracle, cfg)
        self.n = self.t.n_primitives()
        self._m = {}

    def M(self, rays, seed):
        if (rays, seed) not in self._m:
            m = self.o.view_factors(rays, seed=seed, nthreads=8)
            assert m.shape == (self.n, self.n) and m.dtype == np.uint32
            m.setflags(write=False)
            self._m[rays, seed] = m
        return self._m[rays, seed]


def room_world(World, rc, oracle):
    """The closed room of scene_kit.room_cfg as a `World`; freed when the generator is resumed."""
    w = World(rc, oracle, room_cfg(rc))
    assert w.n == 192
    yield w
    w.t.free()
