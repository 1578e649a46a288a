"""The inputs of tests/test_gpu_auto_rebuild.py, checked on the CPU with the oracle alone (tests/auto_rebuild_model.py): under RATIO = 1.5
the six frames decide refit, rebuild, refit, refit, rebuild, refit with room on both sides, and on every frame the tree a rebuild gives
differs from the refitted one in enough leaf slots that a decision taken wrongly, either way, cannot pass a byte comparison."""
import numpy as np
import pytest

import auto_rebuild_model as model

SMALL, LARGE = (6, 6, 4), (12, 12, 6)  # the lattices of tests/test_gpu_dynamic.py


@pytest.fixture(scope="module")
def sc():
    import raycore_jl_amd
    return raycore_jl_amd.scenes


def steps_of(oracle, sc, dims):
    mesh = sc.fan_sphere(10, 6, radius=0.5)
    initial = sc.lattice_transforms(*dims, 1.6, 3)[0]
    n = len(initial)
    frames = model.animation(sc, dims, initial)
    fresh = [model.oracle_nodes(oracle, mesh, xf) for xf in frames]
    return n, frames, fresh, model.walk(model.oracle_nodes(oracle, mesh, initial), fresh, n, lambda topo, f: model.refit(topo, fresh[f], n))


@pytest.mark.parametrize("dims", [SMALL, LARGE], ids=["144", "864"])
def test_conditions_on_the_inputs(oracle, sc, dims):
    n, frames, fresh, steps = steps_of(oracle, sc, dims)
    assert n == int(np.prod(dims)) and len(steps) == 6
    model.assert_conditions(steps, f"{n} instances")
    assert [s["rebuild"] for s in steps] == list(model.REBUILDS)
    for f, s in enumerate(steps):  # a rebuilding frame leaves the fresh tree and its cost, a refitting one keeps the baseline
        if s["rebuild"]:
            assert s["nodes"].tobytes() == fresh[f].tobytes() and s["cost_built"] == model.cost(fresh[f], n)
        else:
            assert s["cost_built"] == s["cost_built_before"] and s["nodes"].tobytes() != fresh[f].tobytes()


def test_refit_of_a_tree_to_its_own_leaves_is_the_tree(oracle, sc):
    """The model's refit restates the oracle's own boxes when nothing moved, and the cost of one leaf is exactly 1."""
    mesh = sc.fan_sphere(10, 6, radius=0.5)
    xf = sc.lattice_transforms(*SMALL, 1.6, 3)[0]
    nodes = model.oracle_nodes(oracle, mesh, xf)
    assert model.refit(nodes, nodes, len(xf)).tobytes() == nodes.tobytes()
    assert model.cost(nodes, len(xf)) > 1.0
    one = model.oracle_nodes(oracle, mesh, xf[:1])
    assert model.cost(one, 1) == 1.0 and model.refit(one, one, 1).tobytes() == one.tobytes()
    two = model.oracle_nodes(oracle, mesh, xf[:2])
    assert model.cost(two, 2) == 1.0  # one internal node: the root
