"""Register / scratch budget of render_fixed_kernel (the step's bulk render launch compiled for 80 x 60 frames), from the
build's resource remarks (scripts/kernel_resources.py; no GPU).  A kernel's name carries <NBOX, POLY, LAYOUT, DEPTH>; each must
fit what the generic bulk kernel render_kernel<256, 2, NBOX, POLY> fits - 96 VGPRs, five workgroups per CU, at most 12 B/lane
of scratch - and, having fewer live scalars, may not reload more SGPRs than that kernel does in the same build."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")

VARIANTS = [(1, False), (2, False), (6, False), (1, True)]   # (NBOX, POLY) of the box tasks


@pytest.fixture(scope="module")
def table():
    from kernel_resources import kernel_resources
    return kernel_resources()


def _true(s):
    return s in ("1", "true")


def _fixed(table):
    out = {}
    for name, r in table.items():
        m = re.search(r"render_fixed_kernelILi(\d+)ELb(\d)ELi(\d)ELb(\d)E", name) or \
            re.search(r"render_fixed_kernel<(\d+), (true|false), (\d), (true|false)>", name)
        if m:
            out[(int(m.group(1)), _true(m.group(2)), int(m.group(3)), _true(m.group(4)))] = r
    return out


def _generic_bulk(table):
    out = {}
    for name, r in table.items():
        m = re.search(r"render_kernelILi256ELi2ELi(\d+)ELb(\d)E", name) or re.search(r"render_kernel<256, 2, (\d+), (true|false)>", name)
        if m:
            out[(int(m.group(1)), _true(m.group(2)))] = r
    return out


def test_all_sixteen_instantiations_are_reported(table):
    want = {(nb, poly, layout, depth) for nb, poly in VARIANTS for layout in (0, 1) for depth in (False, True)}
    assert set(_fixed(table)) == want, sorted(want ^ set(_fixed(table)))


def test_fixed_kernels_fit_the_bulk_budget(table):
    for key, r in _fixed(table).items():
        assert r["vgprs"] <= 96 and r["agprs"] == 0, (key, r)
        assert r["occupancy"] >= 5, (key, r)
        assert r["scratch"] <= 12, (key, r)


def test_no_more_sgpr_spills_than_the_generic_kernel_of_the_same_build(table):
    generic = _generic_bulk(table)
    for (nb, poly, layout, depth), r in _fixed(table).items():
        assert r["sgpr_spill"] <= generic[(nb, poly)]["sgpr_spill"], ((nb, poly, layout, depth), r["sgpr_spill"], generic[(nb, poly)]["sgpr_spill"])
