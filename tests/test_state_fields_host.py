"""CPU: the one list of mwb_state's fields (gym_miniworld_amd/csrc/mwb_state_fields.h) and the get / check / put functions
mwb_get_state and mwb_set_state are made of, run over host arrays with memcpy as the mover (state_fields_host.cpp; built with
AddressSanitizer + UBSan where their runtimes link - a stand-alone program, nothing is preloaded).

Every expected element is computed here from the layout rules alone - per-env arrays are [N][w], per-slot arrays [B][N][w]
planes, mwb_state is [count][w] / [count][B][w], ent_order is padded to 24 bytes per env - and from the program's fill rule:
element i of array number a holds a * 65536 + i (+ 10^9 in the handle that is set, + 0.25 in floating point)."""
import os
import subprocess

import numpy as np
import pytest

from gym_miniworld_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gym_miniworld_amd", "csrc")
N = 5
RANGES = [(1, 3), (0, 5), (2, 0)]
TASKS = {"OneRoom": 1, "TMazeTwoBox": 2, "PutNext": 6, "CollectHealth": None}   # task -> B (None: whatever the entity task has)
ORDER_STRIDE, AGENT = 24, 255
BOX, WRITE, ENT, FINITE, POSITIVE, CODE = 1, 2, 4, 8, 16, 32
DT = {"f8": np.float64, "f4": np.float32, "i4": np.int32, "u4": np.uint32, "i8": np.int64, "u1": np.uint8}
PLANES = {"agent_pos": ("agent_x", None, "agent_z"), "box_pos": ("box_x", "box_y", "box_z")}
ARRAY_OF = {"rng_state": "rng"}   # (every other plain field moves to / from the array of its own name)
ENT_ONLY = "mwb_set_state: entity-list fields exist for the tasks >= MWB_TASK_PICKUPOBJS only"


def exe():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    path, src = os.path.join(out, "state_fields_host"), os.path.join(HERE, "state_fields_host.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("mwb_state_fields.h", "mwb_internal.h", "mwb_task_table.h")]
    if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in deps):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-D__HIP_PLATFORM_AMD__", "-I",
               os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-o", path, src]
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)
    return path


class Host:
    """one run of the program for one task: the model of both handles' arrays beside it"""

    def __init__(self, task):
        self.p = subprocess.Popen([exe(), str(_lib.TASK_IDS[task]), "0", "0", "0", "0", str(N)], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        self.ent = _lib.TASK_IDS[task] >= _lib.ENT_TASK_FIRST
        self.fields = [(f[1], int(f[4]), int(f[5])) for f in self.ask(["table"])]
        self.B = dict((n, w) for n, w, _ in self.fields)["ent_order"] - 1
        self.hashes, self.src, self.dst = {}, {}, {}
        for a, row in enumerate(self.ask(["dump"])):   # the fill rule, restated: the first dump must be it
            name, kind, n = row[1], row[2], int(row[3])
            if row[4] == "hash":
                self.hashes[name] = row[5]
                continue
            base = a * 65536 + np.arange(n, dtype=np.int64)
            if name == "n_order":
                self.src[name] = np.array([self.B + 1 - e % 3 for e in range(N)], np.int32)
                self.dst[name] = self.src[name].copy()
            elif name == "ent_order":
                self.src[name] = np.array([[200 + k if k > self.B else AGENT if k == e % (self.B + 1) else (e + k) % self.B
                                            for k in range(ORDER_STRIDE)] for e in range(N)], np.uint8).reshape(-1)
                self.dst[name] = self.src[name].copy()
            elif kind in ("f8", "f4"):
                self.src[name], self.dst[name] = (base + 0.25).astype(DT[kind]), (base + 1e9 + 0.25).astype(DT[kind])
            else:
                self.src[name], self.dst[name] = base.astype(DT[kind]), (base + 10 ** 9).astype(DT[kind])
            assert n == len(base) and self.same(row[4:], self.dst[name]), name
        assert {"agent_x", "box_color", "rng", "cam"} <= set(self.src) and ("ent_meta" in self.src) == self.ent

    def ask(self, lines):
        self.p.stdin.write("\n".join(lines) + "\n")
        self.p.stdin.flush()
        rows = []
        while True:
            ln = self.p.stdout.readline()
            assert ln, ("the program ended", self.p.stderr.read()[-3000:])
            if ln.strip() == "end":
                return rows
            rows.append(ln.split())

    def close(self):
        self.p.stdin.close()
        assert self.p.wait() == 0, self.p.stderr.read()[-3000:]   # (with the sanitizers: no leak either)

    @staticmethod
    def same(tokens, want):
        got = np.array([float(t) for t in tokens]) if want.dtype.kind == "f" else np.array([int(t) for t in tokens], dtype=np.int64)
        return len(got) == want.size and np.array_equal(got.astype(want.dtype), want.reshape(-1))

    # ---- the layout rules
    def shape(self, name):
        """of one env's part of the field in mwb_state"""
        return tuple({"B": self.B, "B+1": self.B + 1}.get(s, s) for s in next(f[2] for f in _lib.STATE_FIELDS if f[0] == name))

    def at(self, arr, e, b=None, c=0, w=1):
        """flat index of component c of env e (slot b) in a device array of width w"""
        return e * w + c if b is None else (b * N + e) * w + c

    def expected_get(self, dev, name, first, count):
        flags = next(f for n, _, f in self.fields if n == name)
        out = np.zeros((count,) + self.shape(name), next(DT[f[1]] for f in _lib.STATE_FIELDS if f[0] == name))
        for i in range(count):
            e = first + i
            if name in PLANES:
                for c, plane in enumerate(PLANES[name]):
                    if plane is None:
                        continue
                    if flags & BOX:
                        out[i, :, c] = [dev[plane][self.at(plane, e, b)] for b in range(self.B)]
                    else:
                        out[i, c] = dev[plane][self.at(plane, e)]
            elif name == "ent_order":
                row = dev["ent_order"][e * ORDER_STRIDE:(e + 1) * ORDER_STRIDE]
                out[i] = [-1 if k >= dev["n_order"][e] else -2 if row[k] == AGENT else row[k] for k in range(self.B + 1)]
            elif name in ("rng_pos", "rng_keysum"):
                words = dev["rng"][e * 625:(e + 1) * 625].astype(np.uint64)
                out[i] = words[624] if name == "rng_pos" else int(words[:624].sum()) % 2 ** 32
            else:
                arr = dev[ARRAY_OF.get(name, name)]
                w = int(np.prod(self.shape(name)[1:] if flags & BOX else self.shape(name), dtype=np.int64))
                if flags & BOX:
                    out[i] = np.array([[arr[self.at(arr, e, b, c, w)] for c in range(w)] for b in range(self.B)]).reshape(out[i].shape)
                else:
                    out[i] = np.array([arr[self.at(arr, e, None, c, w)] for c in range(w)]).reshape(out[i].shape)
        return out

    def apply_set(self, dev, name, first, values):
        """what a successful mwb_set_state of this field does to the arrays"""
        flags = next(f for n, _, f in self.fields if n == name)
        if not flags & WRITE:
            return
        for i, v in enumerate(values):
            e = first + i
            if name in PLANES:
                for c, plane in enumerate(PLANES[name]):
                    if plane is None:
                        continue
                    for b in range(self.B if flags & BOX else 1):
                        dev[plane][self.at(plane, e, b if flags & BOX else None)] = v[b, c] if flags & BOX else v[c]
            elif name == "ent_order":
                lst = list(v[:list(v).index(-1)] if -1 in v else v)
                dev["ent_order"][e * ORDER_STRIDE:(e + 1) * ORDER_STRIDE] = [AGENT if x == -2 else x for x in lst] + [AGENT] * (ORDER_STRIDE - len(lst))
                dev["n_order"][e] = len(lst)
            else:
                arr = dev[ARRAY_OF.get(name, name)]
                flat = np.asarray(v).reshape(self.B if flags & BOX else 1, -1)
                for b in range(flat.shape[0]):
                    for c in range(flat.shape[1]):
                        arr[self.at(arr, e, b if flags & BOX else None, c, flat.shape[1])] = flat[b, c]

    # ---- requests
    def get(self, first, count, every=False):
        rows = self.ask(["get %d %d%s" % (first, count, " all" if every else "")])
        assert rows[0][0] == "rc" and rows[0][2] == "|"
        return int(rows[0][1]), " ".join(rows[0][3:]), {r[0]: r[1:] for r in rows[1:]}

    def set(self, first, count, fields):
        lines = ["set %d %d" % (first, count)]
        for k, v in fields.items():
            a = np.asarray(v)
            lines.append(k + " " + " ".join(repr(float(x)) if a.dtype.kind == "f" else str(int(x)) for x in a.reshape(-1)))
        rows = self.ask(lines + ["go"])
        return int(rows[0][1]), " ".join(rows[0][3:])

    def check_dump(self):
        """every array of the handle that is set is what the model says"""
        for row in self.ask(["dump"]):
            if row[4] == "hash":
                assert row[5] == self.hashes[row[1]], row[1]
            else:
                assert self.same(row[4:], self.dst[row[1]]), row[1]

    def new_values(self, first, count, names):
        """valid values, distinct per field and element, unlike anything the arrays hold"""
        out = {}
        for k, name in enumerate(names):
            dt = next(DT[f[1]] for f in _lib.STATE_FIELDS if f[0] == name)
            v = (np.arange(int(np.prod((count,) + self.shape(name), dtype=np.int64))) + 5000 + 1000 * k).reshape((count,) + self.shape(name))
            if name == "goal_idx":
                v = v % 2
            elif name == "carrying":
                v = v % (self.B + 1) - 1
            elif name == "rng_state":
                v[:, 624] = [(first + i) * 156 for i in range(count)]   # 0 .. 624
            elif name == "ent_meta" and self.ent:   # the alive bit flipped in every other slot
                v = self.expected_get(self.dst, name, first, count) ^ ((np.arange(v.size).reshape(v.shape) % 2) << 9)
            elif name == "ent_order":  # the agent somewhere, the slots backwards, shorter by i % 4 entries
                for i in range(count):
                    lst = list(range(self.B - 1, -1, -1))
                    lst.insert((first + i) % (self.B + 1), -2)
                    v[i] = (lst[:self.B + 1 - i % 4] + [-1] * 4)[:self.B + 1]
            out[name] = (v + 0.5).astype(dt) if np.dtype(dt).kind == "f" else v.astype(dt)
        return out


@pytest.fixture(scope="module", params=sorted(TASKS))
def host(request):
    h = Host(request.param)
    assert TASKS[request.param] in (None, h.B)
    yield h
    h.close()


def names(h, writable=None):
    return [n for n, _, f in h.fields if (h.ent or not f & ENT) and (writable is None or bool(f & WRITE) == writable)]


def test_the_table_is_the_python_table(host):
    assert [n for n, _, _ in host.fields] == [f[0] for f in _lib.STATE_FIELDS]
    for (name, offset, size, width, flags), (pname, dt, shape, writable, ent) in zip([(r[1],) + tuple(int(x) for x in r[2:]) for r in host.ask(["table"])],
                                                                                    _lib.STATE_FIELDS):
        assert name == pname and offset == getattr(_lib.MwbState, name).offset and size == np.dtype(dt).itemsize, name
        box = bool(shape) and shape[0] == "B"
        assert bool(flags & BOX) == box and bool(flags & WRITE) == writable and bool(flags & ENT) == ent, name
        assert width == int(np.prod(host.shape(name)[1:] if box else host.shape(name), dtype=np.int64)), name
        assert not flags & (FINITE | POSITIVE) or dt == "f8", name
        assert bool(flags & POSITIVE) == (name == "box_size") and bool(flags & CODE) == (name in ("agent_pos", "box_pos", "ent_order", "rng_pos", "rng_keysum")), name
    finite = {"agent_pos", "agent_dir", "box_pos", "box_dir", "box_color", "box_size", "cam", "sky_color", "light_pos", "light_color", "light_ambient", "goal_dist"}
    assert {n for n, _, f in host.fields if f & FINITE} == finite


@pytest.mark.parametrize("first,count", RANGES)
def test_get(host, first, count):
    rc, why, got = host.get(first, count)
    assert (rc, why) == (0, "") and list(got) == names(host)
    for name, tokens in got.items():
        want = host.expected_get(host.src, name, first, count)
        pad = np.frombuffer(b"\x5a" * 8, want.dtype)[:1]   # the element past the end is still the caller's
        assert host.same(tokens, np.concatenate([want.reshape(-1), pad])), name
    if not host.ent:
        rc, why, got = host.get(first, count, every=True)
        assert (rc, why, got) == (-1, "mwb_get_state: entity-list fields exist for the tasks >= MWB_TASK_PICKUPOBJS only", {})


@pytest.mark.parametrize("first,count", RANGES)
def test_set(host, first, count):
    # two arrays only, then everything writable, then the fields mwb_set_state ignores: each time every array is as expected
    for chosen in (["box_color", "agent_dir"], names(host, writable=True), [n for n in names(host, writable=False) if not n.startswith("ent_") and n != "text_tex"]):
        vals = host.new_values(first, count, chosen)
        assert host.set(first, count, vals) == (0, ""), chosen
        for name, v in vals.items():
            host.apply_set(host.dst, name, first, v)
        host.check_dump()


def test_refusals_change_nothing(host):
    first, count, B = 1, 3, host.B
    good = host.new_values(first, count, ["agent_dir", "goal_dist", "box_size", "rng_state", "goal_idx", "carrying"])

    def refused(why, **bad):
        fields = dict(good)
        fields.update(bad)
        assert host.set(first, count, fields) == (-1, why), bad
        host.check_dump()
    cases = [("mwb_set_state: goal_idx must be 0 or 1", dict(goal_idx=[0, 1, 2])), ("mwb_set_state: goal_idx must be 0 or 1", dict(goal_idx=[-1, 0, 0])),
             ("mwb_set_state: carrying must be -1 or a box index", dict(carrying=[0, -1, B])), ("mwb_set_state: carrying must be -1 or a box index", dict(carrying=[-2, 0, 0]))]
    rng = good["rng_state"].copy()
    rng[2, 624] = 625
    cases.append(("mwb_set_state: MT19937 position must be 0..624", dict(rng_state=rng)))
    for name in [n for n, _, f in host.fields if f & FINITE]:
        for bad in (np.nan, np.inf, -np.inf):
            v = host.new_values(first, count, [name])[name]
            v.reshape(-1)[-1] = bad
            cases.append(("mwb_set_state: non-finite value", {name: v}))
    for bad in (0.0, -0.8):
        v = good["box_size"].copy()
        v[1, B - 1] = bad
        cases.append(("mwb_set_state: box_size must be > 0", dict(box_size=v)))
    if host.ent:
        for name in ("ent_radius", "ent_height", "ent_scale", "text_tex"):
            cases.append(("mwb_set_state: ent_radius / ent_height / ent_scale / text_tex are read-only", {name: host.new_values(first, count, [name])[name]}))
        meta = host.new_values(first, count, ["ent_meta"])["ent_meta"]
        for bit in (0, 4, 8, 10, 12):
            v = meta.copy()
            v[2, B - 1] ^= 1 << bit
            cases.append(("mwb_set_state: ent_meta may only change an entity's alive bit", dict(ent_meta=v)))
        order = host.new_values(first, count, ["ent_order"])["ent_order"]
        for col, val, why in ((1, None, "lists an entity twice"), (0, B, "entries are slots, -2 (the agent) or -1 (end)"), (0, -3, "entries are slots, -2 (the agent) or -1 (end)")):
            v = order.copy()
            v[0, col] = v[0, 0] if val is None else val
            cases.append(("mwb_set_state: ent_order " + why, dict(ent_order=v)))
    else:
        for name in ("ent_meta", "ent_radius", "ent_order", "task_f", "task_i", "text_tex"):
            cases.append((ENT_ONLY, {name: host.new_values(first, count, [name])[name]}))
    for why, bad in cases:
        refused(why, **bad)
    assert host.set(first, count, good) == (0, "")   # the same fields without the offending one go through
    for name, v in good.items():
        host.apply_set(host.dst, name, first, v)
    host.check_dump()
