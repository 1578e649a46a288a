"""RcSceneState (raycore.jl_amd/csrc/rc_scene_state.h), the host-side state flags of a mutable scene and their named transitions, beside
the lifecycle model on a CPU.  The header includes no HIP header, so tests/host/scene_state_main.cpp -- which drives one RcSceneState the
way each entry point of the library does: the gate, then the transitions in the entry point's order -- is compiled with the host compiler
under AddressSanitizer / UBSan and run as a child process, one run per walk of lifecycle_model.SEEDS.

Every operation of a walk is expanded into the entry points tests/test_gpu_lifecycle_walk.py issues for it (ENTRY_POINTS below); the
program's answer to each -- ok, not_synced, or the action of a sync -- must be what the model says of the operation.  A refused operation
is refused by the FIRST entry point of its sequence, which is then the only one issued.  Left out: operations the model refuses with
another error than RC_ERR_NOT_SYNCED (invalid handle, invalid argument, the deferred geometry error of wait -- the library returns before
it touches a flag) and the two BLAS4 readers (governed by Blas::n_nodes4, not by these flags).  The program itself checks after every line
that host_instances_stale implies !mirror_edited and that device_dirty implies transforms_dirty."""
import os
import shutil
import subprocess

import pytest

import lifecycle_model as lm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_OPS = 120

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

COMMIT_ENTRY = {"refit": "refit_device_async", "rebuild": "rebuild_tlas_device_async", "gated": "refit_or_rebuild_tlas_device_async"}
EXPORTS = ("export_instances", "export_host", "export_host", "export_host", "export_blas_descs", "export_triangles", "world_bound")
# operation -> the entry points its do_* method in tests/test_gpu_lifecycle_walk.py calls, in order.  A callable gets (op, outcome, model
# after the operation).  Flags behind a name: "empty" (no instance in the scene), "capturing", "gone" (delete of a handle that is not live).
ENTRY_POINTS = {
    "push": ("add_blas", "add_instances"),
    "push_shared": lambda op, out, m: ("add_blas",) + ("add_instances",) * len(op[3]),
    "push_mesh": ("add_blas", "add_instances"),
    "delete": lambda op, out, m: ("delete" if out.value else "delete gone",),
    "update_transforms": ("update_transforms",),
    "update": ("update_geometry",),
    "update_mesh": ("update_geometry",),
    "sync": lambda op, out, m: ("sync empty" if m.n_total() == 0 else "sync", "sync"),  # (the second one must find nothing to do)
    "utd": ("update_transforms_device",),
    "ugd": ("update_geometry_device",),
    "umd": ("update_geometry_device",),
    "ibr": lambda op, out, m: ("instance_buffer_device", "refit_device" if op[3] in (0, 1) else COMMIT_ENTRY[op[3]]),
    "refit": lambda op, out, m: (commit_line("refit", m),),
    "rebuild": lambda op, out, m: (commit_line("rebuild", m),),
    "gated": lambda op, out, m: (commit_line("gated", m),),
    "wait": ("wait",),
    # the chain has just run eagerly; the trace and the attributes once more eagerly, then the chain and a trace into the graph
    "capture": lambda op, out, m: ("trace_device", "shading_attributes_device", "update_transforms_device capturing") +
                                  (("update_geometry_device capturing",) if op[2] else ()) + (COMMIT_ENTRY[op[3]] + " capturing", "trace_device"),
    "replay": ("graph_launch",),  # the graph runs the captured kernels: no entry point of the library is called, no flag moves
    "release": ("release_captures",),
    "get_instances": ("get_instances", "get_instances"),  # (the count, then the records)
    "world_bound": ("world_bound",),
    "exports": EXPORTS,
    "counts": ("counts",),
    "quality": ("tlas_quality",),
    "save_load": ("scene_save",),
    "collide": ("collide_instances",),
    "vf": ("view_factor_totals", "view_factors"),
    "shading": ("trace_device", "shading_attributes_device"),
    "trace": ("trace_host",),
}
LEFT_OUT = ("blas4_build", "blas4_trace")
# of the 1 440 operations of the twelve walks, 133 are left out: 18 + 4 + 6 that end in RC_ERR_INVALID_ARGUMENT / _INVALID_HANDLE /
# _GEOMETRY_CHANGED, and 57 blas4_build + 48 blas4_trace (36 of the 172 RC_ERR_NOT_SYNCED answers of the walks are blas4_trace's)
N_FED, N_REFUSED = 1307, 136


def commit_line(kind, m):
    return COMMIT_ENTRY[kind] + (" empty" if m.n_total() == 0 else "")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_state") / "scene_state")
    base = ["g++", "-std=c++17", "-g", "-I", os.path.join(ROOT, "raycore.jl_amd", "csrc"), os.path.join(HERE, "host", "scene_state_main.cpp"), "-o", exe]
    # (the sanitizer runtimes linked statically: the program then runs the same whatever libraries its environment preloads)
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if p.returncode != 0 and "san" in p.stderr and "scene_state_main.cpp:" not in p.stderr:  # no sanitizer runtime on this machine: the plain build still checks the rules
        p = subprocess.run(base, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def script(ops):
    """-> ([(operation index, entry-point line, expected answer)], operations fed, sync actions, refusals)"""
    lines, fed, actions, refused = [], 0, [], 0

    def on_outcome(k, op, out, model):
        nonlocal fed, refused
        if op[0] in LEFT_OUT or out.error not in (None, lm.RC_ERR_NOT_SYNCED):
            return
        fed += 1
        seq = ENTRY_POINTS[op[0]]
        seq = seq(op, out, model) if callable(seq) else seq
        if out.error == lm.RC_ERR_NOT_SYNCED:
            refused += 1
            lines.append((k, seq[0], "not_synced"))
        elif op[0] == "sync":
            actions.append(out.action)
            lines.extend([(k, seq[0], out.action), (k, seq[1], "noop")])
        else:
            lines.extend((k, e, "ok") for e in seq)

    lm.run(ops, on_outcome=on_outcome)
    return lines, fed, actions, refused


def test_walks_against_the_model(exe):
    total = fed_total = refused_total = 0
    actions = []
    for regime, seeds in lm.SEEDS.items():
        for seed in seeds:
            ops = lm.walk(seed, regime, N_OPS)
            lines, fed, acts, refused = script(ops)
            total, fed_total, refused_total = total + len(ops), fed_total + fed, refused_total + refused
            actions += acts
            r = subprocess.run([exe], input="".join(e + "\n" for _, e, _ in lines), capture_output=True, text=True)
            got = r.stdout.split()
            for (k, entry, want), answer in zip(lines, got):
                assert answer == want, f"{entry}: the scene state answers {answer}, the model says {want}\n{lm.describe(seed, regime, ops, k)}"
            assert r.returncode == 0 and len(got) == len(lines), f"seed {seed}, regime {regime}: exit status {r.returncode}\n{r.stderr[-3000:]}"
    assert total == 12 * N_OPS
    assert fed_total == N_FED and fed_total >= 0.9 * total, (fed_total, total)
    # the walks reach every answer: refusals, and each of the three things a sync can do
    assert refused_total == N_REFUSED, refused_total
    assert {a: actions.count(a) for a in ("rebuild", "refit", "noop")} == {"rebuild": 109, "refit": 37, "noop": 2}, actions


def test_flags_are_private(tmp_path):
    """A write of a flag from outside the header does not compile."""
    src = tmp_path / "raw_write.cpp"
    src.write_text('#include "rc_scene_state.h"\nint main() { RcSceneState s; s.f.dirty = false; return s.synced(); }\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "raycore.jl_amd", "csrc"), str(src)], capture_output=True, text=True)
    assert p.returncode != 0 and "private" in p.stderr, p.stderr[-2000:]
