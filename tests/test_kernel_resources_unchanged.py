"""The kernels that take no part in the texel pipelining of the fixed-shape bulk kernels - every render_kernel,
render_grey_kernel, render_view_kernel and reset_kernel instantiation - must come out of the compiler as their parent commit
left them: VGPRs, SGPR spills, scratch and occupancy from the build's resource remarks (scripts/kernel_resources.py; no GPU)
equal the values recorded from the parent in tests/golden/kernel_resources_parent.json (the same script's output there)."""
import json
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")

GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_parent.json")
FIELDS = ("vgprs", "sgpr_spill", "scratch", "occupancy")
FAMILIES = ("render_kernel", "render_grey_kernel", "render_view_kernel", "reset_kernel")


def canon(name):
    """'render_kernel<256,2,1,0>' from either spelling of a kernel's name: demangled ('void render_kernel<256, 2, 1, false>(MwbDev)')
    or, where no demangler is installed, mangled ('_Z13render_kernelILi256ELi2ELi1ELb0EEv6MwbDev'); None for other names"""
    m = re.match(r"_Z(\d+)", name)
    if m:
        base = name[m.end():m.end() + int(m.group(1))]
        args = re.match(r"I((?:L[ib]\d+E)+)E", name[m.end() + int(m.group(1)):])
        vals = re.findall(r"L[ib](\d+)E", args.group(1)) if args else None
    else:
        m = re.match(r"(?:void )?(\w+)<([^>]*)>", name)
        base = m.group(1) if m else None
        vals = [{"true": "1", "false": "0"}.get(a.strip(), a.strip()) for a in m.group(2).split(",")] if m else None
    return "%s<%s>" % (base, ",".join(vals)) if vals else None


def family(key):
    return key.split("<")[0]


@pytest.fixture(scope="module")
def table():
    from kernel_resources import kernel_resources
    return {canon(k): v for k, v in kernel_resources().items() if canon(k) and family(canon(k)) in FAMILIES}


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    assert re.fullmatch(r"[0-9a-f]{40}", g["parent_commit"])
    return g["kernels"]


def test_the_fixture_covers_every_family(parent):
    assert {family(k) for k in parent} == set(FAMILIES)
    assert all(set(v) == set(FIELDS) for v in parent.values())


def test_same_kernels_as_the_parent(table, parent):
    assert set(table) == set(parent), sorted(set(table) ^ set(parent))


def test_resources_equal_the_parents(table, parent):
    diff = {k: ({f: table[k][f] for f in FIELDS}, parent[k]) for k in parent if k in table and {f: table[k][f] for f in FIELDS} != parent[k]}
    assert not diff, diff
