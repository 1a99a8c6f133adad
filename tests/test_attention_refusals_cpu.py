"""What the six attention entries refuse, recorded field by field: one good argument set per entry is made bad one field at
a time and every bad set must come back CS_EINVAL before anything else happens -- no launch, no HIP call, so this runs without
a GPU (after test_abi_cpu.test_every_entry_rejects_null_arguments_without_touching_the_device).  Pointers are integers that
are never dereferenced.

One case cannot stay in this process: a workspace that is off by 4 bytes is IGNORED, alignment included, where the image
route does not apply (cs_attn_f16x3_ws_bytes == 0), so that call gets past the check and reaches the launch.  It runs in a
child process that sees no GPU (and says so before it calls), where the launch fails with a HIP error: not CS_EINVAL, not
CS_OK."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
P = 0x10000000                      # q; k, v, out, status, ws follow 1 MiB apart (all 16-byte aligned, none ever read)
PTRS = dict(q=P, k=P + (1 << 20), v=P + (2 << 20), out=P + (3 << 20), status=P + (4 << 20), ws=P + (5 << 20))
SMALL = dict(nb=1, nq=8, nk=8, heads=2, dh=4, ldq=8, ldk=8, ldv=8, ldo=8)
IMAGE = dict(nb=1, nq=1024, nk=128, heads=1, dh=132, ldq=132, ldk=132, ldv=132, ldo=132)     # the tile-image route
SCALES = dict(q_scale=8.0, k_scale=32.0, v_scale=4.0)
HEAD = ["q", "k", "v", "out", "nb", "nq", "nk", "heads", "dh", "ldq", "ldk", "ldv", "ldo", "scale"]
ENTRIES = {      # name -> argument order (include/commonscenes_hip.h)
    "cs_attn_selfattn": HEAD + ["stream"],
    "cs_attn_selfattn_f16x3": HEAD + ["status", "stream"],
    "cs_attn_selfattn_f16": HEAD + ["status", "stream"],
    "cs_attn_selfattn_f16x3_scaled": HEAD + ["q_scale", "k_scale", "v_scale", "status", "stream"],
    "cs_attn_selfattn_f16x3_ws": HEAD + ["status", "ws", "stream"],
    "cs_attn_selfattn_f16x3_ws_scaled": HEAD + ["q_scale", "k_scale", "v_scale", "status", "ws", "stream"],
}


def good_sets(name):
    base = dict(PTRS, scale=0.5, stream=None, **SCALES)
    sets = [("small", dict(base, **SMALL))]
    if name.endswith(("_ws", "_ws_scaled")):
        sets.append(("image", dict(base, **IMAGE)))
    return sets


def bad_fields(name, good):
    """(label, changed fields) of every refusal the entry owes for this good set"""
    hd = good["heads"] * good["dh"]
    bad = [(f"{p} null", {p: None}) for p in ("q", "k", "v", "out")]
    bad += [(f"{n} = {x}", {n: x}) for n in ("nb", "nq", "nk", "heads", "dh") for x in (0, -1)]
    bad += [("dh = 6", dict(dh=6))]
    bad += [(f"{ld} odd by 2", {ld: good[ld] + 2}) for ld in ("ldq", "ldk", "ldv", "ldo")]
    bad += [(f"{ld} = heads*dh - 4", {ld: hd - 4}) for ld in ("ldq", "ldk", "ldv", "ldo")]
    bad += [(f"{p} off by 4 bytes", {p: good[p] + 4}) for p in ("q", "k", "v", "out")]
    # past the widest head: alone, and with rows wide enough that the head width is the only thing wrong
    bad += [("dh = 260", dict(dh=260)),
            ("dh = 260, ld to match", dict(dh=260, **{ld: good["heads"] * 260 for ld in ("ldq", "ldk", "ldv", "ldo")}))]
    if "scaled" in name:
        bad += [(f"{s} = {x}", {s: x}) for s in ("q_scale", "k_scale", "v_scale") for x in (0.0, -1.0, math.nan)]
    return bad


def call(dll, name, vals):
    return getattr(dll, name)(*[vals[a] for a in ENTRIES[name]])


def test_the_six_entries_are_the_attention_entries_of_the_abi():
    from commonscenes_amd import lib
    for name, order in ENTRIES.items():
        assert len(lib.SIGNATURES[name][1]) == len(order), name


@pytest.mark.parametrize("name", list(ENTRIES))
def test_each_bad_field_is_refused_before_anything_else(name):
    from commonscenes_amd import lib
    dll = lib.load()
    checked = 0
    for tag, good in good_sets(name):
        for label, change in bad_fields(name, good):
            rc = call(dll, name, dict(good, **change))
            assert rc == lib.CS_EINVAL, f"{name} [{tag}] {label} -> {rc}"
            checked += 1
    assert checked >= 29


def ws_cases(dll):
    """(entry, tag, good set, workspace bytes of its shape) of every workspace entry and good set"""
    out = []
    for name in ENTRIES:
        if "ws" not in ENTRIES[name]:
            continue
        for tag, good in good_sets(name):
            out.append((name, tag, good, dll.cs_attn_f16x3_ws_bytes(*[good[a] for a in ("nb", "nq", "nk", "heads", "dh")])))
    return out


def test_a_misaligned_workspace_is_refused_where_the_image_route_takes_it_and_ignored_elsewhere():
    from commonscenes_amd import lib
    dll = lib.load()
    cases = ws_cases(dll)
    assert any(b == 0 for *_, b in cases)
    if not lib.debug().no_attn_img:
        assert any(b > 0 for *_, b in cases), "the image good set must be on the image route"
    for name, tag, good, nbytes in cases:
        if nbytes > 0:
            rc = call(dll, name, dict(good, ws=good["ws"] + 4))
            assert rc == lib.CS_EINVAL, f"{name} [{tag}] ws off by 4 bytes -> {rc}"
    # ws_bytes == 0: past the check, into a launch that has to fail -- in a child that sees no GPU
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), str(Path(__file__).resolve())],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == sum(1 for *_, b in cases if b == 0)
    for key, rc in got.items():
        assert rc != lib.CS_EINVAL and rc != lib.CS_OK, f"{key} ws off by 4 bytes, ws_bytes == 0 -> {rc}"


def _child():
    """the calls that get past the check; refuses to make them if this process can see a GPU"""
    sys.path.insert(0, str(ROOT))
    from commonscenes_amd import lib
    dll = lib.load()
    n = C.c_int(0)
    count = dll.hipGetDeviceCount          # the HIP runtime the library links, found through its handle
    count.restype, count.argtypes = C.c_int, [C.POINTER(C.c_int)]
    rc = count(C.byref(n))
    if rc == 0 and n.value > 0:
        print(f"this process sees {n.value} GPU(s): not launching on made-up pointers")
        return 1
    got = {}
    for name, tag, good, nbytes in ws_cases(dll):
        if nbytes == 0:
            got[f"{name} [{tag}]"] = call(dll, name, dict(good, ws=good["ws"] + 4))
    print(json.dumps(got))
    return 0


if __name__ == "__main__":
    sys.exit(_child())
