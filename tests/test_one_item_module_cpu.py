"""Kernel 4's one-item module against the general module, offline (no GPU: pcl_jit_prebuild compiles with hiprtc alone): for config 3 at order 4
both are compiled into a temporary directory and their code objects read with the ROCm llvm-readelf, as lab/probes/module_stats.py does.  The
one-item kernel must be smaller, spill fewer scalar registers and use no scratch.  Only the two modules of this test are compared: the measured
numbers are in DESIGN.md 4.2."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import piccolo_jl_amd as pa
from piccolo_jl_amd import _lib, synthetic

KERNEL = "pcl_fused_sparse_kernel"


def _readelf():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "lib", "llvm", "bin", "llvm-readelf")):
            return os.path.join(root, "lib", "llvm", "bin", "llvm-readelf")
    pytest.fail("llvm-readelf of the ROCm installation not found")


def _module_stats(L, what, out_dir):
    """{text bytes, sgpr_spill_count, vgpr_spill_count, private_segment_fixed_size} of pcl_fused_sparse_kernel in the module `what`."""
    s = synthetic.config_system(3)
    G0 = np.ascontiguousarray(np.asarray(s.G_drift, dtype=np.float64).T[None])
    Gj = np.ascontiguousarray(np.stack([np.asarray(g, dtype=np.float64).T for g in s.G_drives_array()]))
    os.makedirs(out_dir)
    rc = L.pcl_jit_prebuild(G0.shape[-1] // 2, Gj.shape[0], G0.ctypes.data, 1, Gj.ctypes.data, 2, what, out_dir.encode())
    assert rc == 0, L.pcl_last_error(None).decode()
    files = glob.glob(os.path.join(out_dir, "*.hsaco"))
    assert len(files) == 1, files
    blob = open(files[0], "rb").read()
    n = int.from_bytes(blob[4:8], "little")  # "PCL2" | u32 name length | u64 code length | u64 checksum | name | code
    co = files[0] + ".co"
    with open(co, "wb") as f:
        f.write(blob[24 + n :])
    readelf = _readelf()
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    # the kernel's entry of amdhsa.kernels: from its .name line to the next kernel's (the keys of an entry are sorted: .name stands in the middle, so
    # the entry is cut at the list markers)
    entries = [e for e in re.split(r"\n\s*- ", notes) if re.search(r"\.name:\s+%s\s" % KERNEL, e)]
    assert len(entries) == 1, len(entries)
    out = {}
    for key in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
        mt = re.search(r"\.%s:\s+(\d+)" % key, entries[0])
        assert mt, key
        out[key] = int(mt.group(1))
    syms = subprocess.run([readelf, "-s", "-W", co], capture_output=True, text=True, check=True).stdout
    sizes = {int(w[2], 0) for w in (l.split() for l in syms.splitlines()) if len(w) >= 8 and w[3] == "FUNC" and w[7] == KERNEL}
    assert len(sizes) == 1, sizes
    out["text"] = sizes.pop()
    return out


def test_one_item_module_is_leaner_than_the_general_module(tmp_path):
    pa.build_library()
    L = _lib.load()
    L.pcl_jit_prebuild.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
    general = _module_stats(L, 0, str(tmp_path / "general"))
    one = _module_stats(L, 7, str(tmp_path / "one_item"))
    print("general module:", general)
    print("one-item module:", one)
    assert 0 < one["text"] < general["text"]
    assert one["sgpr_spill_count"] < general["sgpr_spill_count"]
    assert one["private_segment_fixed_size"] == 0
