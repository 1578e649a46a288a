"""What the CPU-side *_api.py tests share: the plain `rc` fixture (the package, no device needed) and the texts they read -- the C
header, its prototypes, and the Julia binding."""
import functools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rc():
    import raycore_jl_amd
    return raycore_jl_amd


@functools.lru_cache(maxsize=None)
def header():
    return open(os.path.join(ROOT, "include", "raycore_mi355x.h")).read()


def prototype(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()[:-1]) for a in m.group(1).split(",")]  # the types, parameter names dropped


@functools.lru_cache(maxsize=None)
def julia_text():
    return open(os.path.join(ROOT, "raycore.jl_amd", "julia", "RaycoreMI355X.jl")).read()
