#!/usr/bin/env python3
"""Build libsilent_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python pysilent_amd/csrc/build.py [--force] [--verbose] [--out PATH] [-D...]
    python pysilent_amd/csrc/build.py --host-asan     # CPU container only: lib/libsilent_hostonly_asan.so, the HOST side of
                                                      # the library under -fsanitize=address,undefined (silent_host_shim.h)

The library is one translation unit per kernel family (UNITS); they compile side by side, and a unit is recompiled only when
one of the files its last compilation read (hipcc -MMD) is newer than its object -- an A/B build of one kernel header costs one
unit.  Objects and dependency files live in csrc/build/ (git-ignored); `--out` + `-D` flags build a variant library from
objects of its own (build/<name of the library>/).
"""
import concurrent.futures
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
OUT = os.path.join(PKG, "lib", "libsilent_hip.so")
UNITS = ["silent_core", "silent_conv_api", "silent_gray_api", "silent_gray16_api", "silent_peaks_api", "silent_rgb_api", "silent_pyramid_api", "silent_displayer_api"]
HOST_ASAN_OUT = os.path.join(PKG, "lib", "libsilent_hostonly_asan.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "-fno-slp-vectorize",
         "-Wall", "-Wextra", "-Wno-unused-parameter"]


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _deps(depfile):
    """The prerequisites a `-MMD` dependency file lists."""
    try:
        text = open(depfile).read()
    except OSError:
        return None
    text = text.replace("\\\n", " ")
    return [p for p in text.split(":", 1)[1].split() if p]


def _stale(obj, depfile, stamp):
    if not os.path.exists(obj):
        return True
    deps = _deps(depfile)
    if deps is None:
        return True
    t = os.path.getmtime(obj)
    try:
        return any(os.path.getmtime(d) > t for d in deps) or open(stamp).read() != _stamp_text
    except OSError:
        return True


_stamp_text = ""


def build(force=False, verbose=False, out=OUT, defines=()):
    """Compile the stale units (in parallel) and link.  Returns the path of the library."""
    global _stamp_text
    variant = "" if out == OUT else os.path.splitext(os.path.basename(out))[0]
    objdir = os.path.join(HERE, "build", variant)
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    flags = FLAGS + list(defines) + (["-Rpass-analysis=kernel-resource-usage"] if verbose else [])
    _stamp_text = " ".join(flags)          # a change of flags recompiles everything
    jobs = []
    for u in UNITS:
        obj, dep, stamp = (os.path.join(objdir, u + ext) for ext in (".o", ".d", ".flags"))
        if force or _stale(obj, dep, stamp):
            jobs.append((u, [hipcc()] + flags + ["-MMD", "-MF", dep, "-c", os.path.join(HERE, u + ".hip"), "-o", obj], stamp))

    def run(job):
        u, cmd, stamp = job
        t0 = time.time()
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=not verbose, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s.hip:\n%s" % (u, (r.stderr or "") + (r.stdout or "")))
        if r.stderr and not verbose:
            sys.stderr.write(r.stderr)
        with open(stamp, "w") as f:
            f.write(_stamp_text)
        return u, time.time() - t0

    if jobs:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as pool:
            for u, dt in pool.map(run, jobs):
                if verbose or os.environ.get("SILENT_BUILD_TIMES"):
                    print("  %-20s %5.1f s" % (u, dt), flush=True)
    objs = [os.path.join(objdir, u + ".o") for u in UNITS]
    if jobs or not os.path.exists(out) or any(os.path.getmtime(o) > os.path.getmtime(out) for o in objs):
        subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
    return out


# the host side under the sanitizers: no GPU code, kernel launches compiled out (silent_host_shim.h)
HOST_ASAN_FLAGS = ["--offload-host-only", "-cuid=silenthost", "-DSILENT_HOST_ONLY", "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17",
                   "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused-parameter",
                   "-Wno-unused-variable", "-Wno-unused-but-set-variable"]
# tests/gray_bytes_host_main.cpp, once per frame type: the entry-point suffix and the bytes of one frame pixel
HOST_DRIVERS = {"u8": ["-DSILENT_SFX=_u8", "-DSILENT_FRAME_BYTES=1"], "u8x3": ["-DSILENT_SFX=_u8x3", "-DSILENT_FRAME_BYTES=3"],
                "f32": ["-DSILENT_FRAME_BYTES=4"], "view": [], "u16": [], "rgb8": [], "rgb8_view": [], "rgb_nv12": [], "rgb_p010": [], "rgb_yuv": [], "rgb_yuv16": [], "rgb_bayer": [], "plan_tables": [], "kp_tables": [], "attn_tables": [], "rgb_h": []}
# "view": the strided *_view entry points have a driver of their own (both channel counts in one program); "u16": so have the twelve
# uint16 entry points (*_u16 and *_view16); "rgb8": and silent_pyramid_rgb8[_dev] (uint8 colour frames of 3-channel plans); "rgb8_view": and silent_pyramid_rgb8_view[_dev] (strided
# views of such frames, with the walk loader's address enumeration); "rgb_nv12": and silent_pyramid_nv12[_dev] / silent_nv12_to_rgb[_dev]
# (NV12 surfaces, with the same enumeration for the luma and chroma planes); "rgb_p010": and silent_pyramid_p010[_dev] /
# silent_p010_to_rgb[_dev] (P010 / P012 / P016 surfaces: uint16 elements, the enumeration with element alignment); "rgb_yuv": and
# silent_pyramid_yuv[_dev] / silent_yuv_to_rgb[_dev] (planar and packed 8-bit YUV: three planes, the merged staging, the enumeration
# per layout); "rgb_bayer": and silent_pyramid_bayer[_dev] / silent_bayer_to_rgb[_dev] (raw Bayer mosaics: the enumeration of the three-row loader with its neighbour columns); "rgb_yuv16": and silent_pyramid_yuv16[_dev] / silent_yuv16_to_rgb[_dev] (the same for uint16 elements: even offsets); "plan_tables": and silent_pyramid_plan_create_ex (every scalar and table of a plan as text, its allocation-failure exits under LeakSanitizer); "kp_tables": and the keypoint tail's host planning (region tables, summary geometry, workspace layout, cell tables, boost parameters as text); "attn_tables": and
# silent_attention_tail[_dev] / silent_attention_extents (argument validation, the planned tables of the two launches and the workspace layout as text); "rgb_h": and
# silent_rgb_line_end_h[_dev] / silent_rgb_keypoints_h[_dev] (every refusal of the float16-storage RGB entry points in order, beside their float32 twins')
HOST_DRIVER_SOURCES = {"view": "gray_view_host_main.cpp", "u16": "gray_u16_host_main.cpp", "rgb8": "rgb8_host_main.cpp",
                       "rgb8_view": "rgb8_view_host_main.cpp", "rgb_nv12": "rgb_nv12_host_main.cpp", "rgb_p010": "rgb_p010_host_main.cpp", "rgb_yuv": "rgb_yuv_host_main.cpp",
                       "rgb_yuv16": "rgb_yuv16_host_main.cpp", "rgb_bayer": "rgb_bayer_host_main.cpp", "plan_tables": "plan_tables_host_main.cpp", "kp_tables": "kp_tables_host_main.cpp", "attn_tables": "attention_tail_host_main.cpp", "rgb_h": "rgb_h_host_main.cpp"}


def _fresh(out, dep):
    """True when `out` exists and none of the files its compilation read (dependency file `dep`) is newer."""
    deps = _deps(dep) if os.path.exists(out) else None
    return deps is not None and all(os.path.exists(d) and os.path.getmtime(d) <= os.path.getmtime(out) for d in deps)


def build_host_asan(force=False):
    """The host code of the library without a GPU behind it (kernel launches compiled out, device memory = host memory), with
    AddressSanitizer + UndefinedBehaviorSanitizer, as ONE translation unit (silent_unity.hip includes them all).  Never loaded by
    the product; tests/test_sanitizers.py runs it in a python started with LD_PRELOAD=<clang's asan runtime>."""
    dep = os.path.join(HERE, "build", "hostonly_asan.d")
    os.makedirs(os.path.dirname(dep), exist_ok=True)
    if not force and _fresh(HOST_ASAN_OUT, dep):
        return HOST_ASAN_OUT
    os.makedirs(os.path.dirname(HOST_ASAN_OUT), exist_ok=True)
    subprocess.check_call([hipcc()] + HOST_ASAN_FLAGS + ["-fPIC", "-shared", "-fvisibility=hidden", "-shared-libsan", "-Wl,-Bsymbolic", "-MMD",
                                                         "-MF", dep, "-o", HOST_ASAN_OUT, os.path.join(HERE, "silent_unity.hip")])
    return HOST_ASAN_OUT


def build_host_driver(family, force=False):
    """tests/gray_bytes_host_main.cpp (tests/gray_view_host_main.cpp for "view", tests/gray_u16_host_main.cpp for "u16", tests/rgb8_host_main.cpp for "rgb8", tests/rgb8_view_host_main.cpp for "rgb8_view", tests/rgb_nv12_host_main.cpp for "rgb_nv12", tests/rgb_p010_host_main.cpp for "rgb_p010", tests/rgb_yuv_host_main.cpp for "rgb_yuv", tests/rgb_yuv16_host_main.cpp for "rgb_yuv16", tests/plan_tables_host_main.cpp for "plan_tables", tests/kp_tables_host_main.cpp for "kp_tables", tests/attention_tail_host_main.cpp for "attn_tables") + the library's host side as one stand-alone executable under the same sanitizers (the runtime
    is linked in: it is run as a child process, nothing of it is loaded into Python), for one frame type of HOST_DRIVERS.  Returns the
    path of the executable, build/gray_host_<family>; rebuilt when a file it was compiled from is newer."""
    exe = os.path.join(HERE, "build", "gray_host_" + family)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if force or not _fresh(exe, exe + ".d"):
        cmd = [hipcc()] + HOST_ASAN_FLAGS + HOST_DRIVERS[family] + ["-MMD", "-MF", exe + ".d", "-o", exe,
                                                                    os.path.join(os.path.dirname(PKG), "tests", HOST_DRIVER_SOURCES.get(family, "gray_bytes_host_main.cpp"))]
        c = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if c.returncode != 0:
            raise RuntimeError("hipcc failed on the host driver (%s):\n%s" % (family, c.stdout[-4000:]))
    return exe


def asan_runtime():
    """Path of the sanitizer runtime the host-only build needs preloaded (clang's, from the ROCm LLVM)."""
    out = subprocess.check_output([hipcc(), "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


if __name__ == "__main__":
    if "--host-asan" in sys.argv:
        print(build_host_asan(force="--force" in sys.argv))
        sys.exit(0)
    out = OUT
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv, out=out,
                defines=[a for a in sys.argv[1:] if a.startswith("-D")]))
