#!/usr/bin/env python3
"""Build libaum_hip.so for gfx950 with hipcc (no GPU needed to compile).  In-tree output so the .so
travels with the gpurun snapshot:  audio-mamba-aum_amd/aum_hip/libaum_hip.so"""
import concurrent.futures as cf
import hashlib
import re
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(os.path.dirname(HERE), "aum_hip")
OBJ_DIR = os.path.join(HERE, "_obj")
SRC = os.path.join(HERE, "aum_hip.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
         "-Wno-unused-function", "-Wno-unused-variable", "-Rpass-analysis=kernel-resource-usage"] + os.environ.get("AUM_EXTRA_CXXFLAGS", "").split()


def dep_files():
    """what the digest covers: every *.h / *.inc / *.hip of this directory, from a sorted listing (a new header is covered the day it is
    added), and the public header"""
    return sorted(f for f in os.listdir(HERE) if f.endswith((".h", ".inc", ".hip"))) + [os.path.join("..", "..", "include", "aum_hip.h")]


def resource_records(log):
    """the kernels of one hipcc run, from its -Rpass-analysis=kernel-resource-usage remarks: [(function name, scratch bytes per lane)], the
    second None where the record has no scratch line that reads as one"""
    out = []
    for ln in log.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            out.append((m.group(1), None))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and out:
            out[-1] = (out[-1][0], int(m.group(1)))
    return out


def spilling_kernels(log):
    """kernels of one hipcc run that use scratch memory: [(name, bytes per lane)].
    Checked for the kernels of scan_tm_kernels.h and gemm_kernels.h / gemm_ps_kernels.h (COUNTED below), which order their global -> LDS
    loads and stores with HAND-COUNTED `s_waitcnt vmcnt(n)` (memory operations complete in issue order; n = the operations younger than the
    data a wait is for); the channel-major kernels wait through the compiler and may spill.  A register
    spill's scratch_load / scratch_store is one more vector-memory operation the counts do not know about: every wait behind it is short by
    one and the kernel reads tiles that have not landed -- oracle tests at small shapes may still pass, results stop being bitwise repeatable
    (profiles/r06_scan_grid_shift.txt: k_scant_bwd sits at 254 of 256 registers)."""
    return [(name, scratch) for name, scratch in resource_records(log) if scratch and COUNTED.search(name)]


def check_counted_seen(obj, log):
    """raise unless the guard above has really looked at `obj`: every record of its log has a scratch field that parsed, and each kernel
    family that EXPECTED puts into this object has at least one record.  A remark format that changed or a counted kernel that was renamed
    would otherwise let spilling_kernels() return [] for want of a match.  Returns the counted records it saw."""
    recs = resource_records(log)
    unread = [name for name, scratch in recs if scratch is None]
    if unread:
        raise RuntimeError(f"{obj}: resource-usage records without a readable ScratchSize line (has the remark format changed?): {unread[:4]}")
    for prefix, families in EXPECTED.items():
        for fam in families if obj.startswith(prefix) else ():
            if not any(fam in name for name, _ in recs):
                raise RuntimeError(f"{obj}: no resource-usage record of a {fam}* kernel -- the no-scratch guard has nothing to look at")
    return [name for name, _ in recs if COUNTED.search(name)]


COUNTED = re.compile(r"k_scant_|k_gemm_tn|k_gemm_wgrad")
EXPECTED = {"scantm_": ("k_scant_",), "gemm.": ("k_gemm_tn", "k_gemm_wgrad")}          # object name prefix -> counted kernel families it must report


def _digest():
    h = hashlib.sha256()
    for d in dep_files():
        with open(os.path.join(HERE, d), "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def parts():
    out = []
    for part in (1, 2):
        for dt in (0, 1, 2):
            out.append((f"scan_p{part}_d{dt}.o", [f"-DAUM_API_PART={part}", f"-DAUM_DTYPE_ONLY={dt}"]))
    for part in (5, 6):
        for dt in (0, 1, 2):
            out.append((f"scantm_p{part}_d{dt}.o", [f"-DAUM_API_PART={part}", f"-DAUM_DTYPE_ONLY={dt}"]))
    for dt in (1, 2):
        out.append((f"proj_d{dt}.o", ["-DAUM_API_PART=4", f"-DAUM_DTYPE_ONLY={dt}"]))
    out.append(("api.o", ["-DAUM_API_PART=3"]))
    out.append(("gemm.o", ["@gemm.hip"]))          # its own translation unit (plain HIP: MFMA + LDS-DMA, no wave.h)
    return out


def build(force=False, verbose=False):
    os.makedirs(OBJ_DIR, exist_ok=True)
    os.makedirs(OUT_DIR, exist_ok=True)
    so = os.path.join(OUT_DIR, "libaum_hip.so")
    stamp = os.path.join(OBJ_DIR, "digest")
    dig = _digest()
    if not force and os.path.exists(so) and os.path.exists(stamp) and open(stamp).read() == dig:
        return so

    def cc(item):
        name, defs = item
        src = SRC
        if defs and defs[0].startswith("@"):
            src, defs = os.path.join(HERE, defs[0][1:]), defs[1:]
        cmd = [HIPCC] + FLAGS + defs + ["-c", src, "-o", os.path.join(OBJ_DIR, name)]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        return name, r.returncode, r.stdout + r.stderr

    with cf.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        res = list(ex.map(cc, parts()))
    for name, rc, log in res:
        if rc != 0:
            sys.stderr.write(log)
            raise RuntimeError(f"hipcc failed on {name}")
        seen = check_counted_seen(name, log)          # also with AUM_ALLOW_SPILLS: that tolerates spills, not a guard that saw nothing
        if verbose and seen:
            print(f"{name}: no-scratch guard read {len(seen)} counted kernels", flush=True)
        spills = spilling_kernels(log)
        if spills and os.environ.get("AUM_ALLOW_SPILLS") != "1":        # (timing-only ablation builds may set AUM_ALLOW_SPILLS=1)
            raise RuntimeError(f"{name}: kernels that spill registers to scratch memory -- their counted vmcnt waits are wrong: {spills}")
        if verbose and log.strip():
            print("\n".join(ln for ln in log.splitlines() if "kernel-resource-usage" not in ln and "remark:" not in ln))
    objs = [os.path.join(OBJ_DIR, n) for n, _ in parts()]
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so] + objs)
    with open(stamp, "w") as f:
        f.write(dig)
    return so


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
