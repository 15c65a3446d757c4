"""CPU: the list of device allocations a handle owns (gym_miniworld_amd/csrc/mwb_alloc_list.h), built into a host program over
malloc / free (alloc_list_host.cpp): a mark and a release free exactly what came between, one pointer can go from the middle,
releasing twice is harmless, and the destroy path leaves nothing - which AddressSanitizer's leak check at exit confirms where
its runtime links (a stand-alone program: nothing is preloaded)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gym_miniworld_amd", "csrc")


def test_mark_release_and_destroy():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "alloc_list_host")
    srcs = [os.path.join(HERE, "alloc_list_host.cpp"), os.path.join(CSRC, "mwb_alloc_list.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, srcs[0]]
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    assert res.stdout.split("\n")[:3] == ["ok mark_release", "ok release_one", "ok destroy"]


def test_the_api_frees_device_memory_from_the_list_only():
    """mwb_api.hip: one hipMalloc (dev_alloc's) and two hipFree (dev_alloc's own failure path, dev_free)"""
    api = open(os.path.join(CSRC, "mwb_api.hip")).read()
    assert api.count("hipMalloc(") == 1 and api.count("hipFree(") == 2
    assert "h->mem.release_to(0, dev_free)" in api
