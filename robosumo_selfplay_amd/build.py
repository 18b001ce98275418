"""Build the in-tree HIP libraries for gfx950 (hipcc cross-compiles without a GPU)."""
import os
import shutil
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
ARCH = "gfx950"


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build the HIP engine")
    return exe


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def lib_path(name):
    return os.path.join(_CSRC, name)


ROLLOUT_SHARDS = 5    # sumo_engine.hip: one object per dynamic-layout variant of the rollout kernel (SUMO_ROLLOUT_SHARD) + one for the rest


def _workers():
    n = os.environ.get("MAX_JOBS") or os.environ.get("CMAKE_BUILD_PARALLEL_LEVEL")
    return max(1, min(int(n) if n else (os.cpu_count() or 1), 16))


def build_all(force=False, verbose=False):
    """Compile every HIP translation unit into its shared library. Returns the list of built paths.

    One translation unit compiles on one core, and sumo_engine.hip's rollout kernels take minutes there: the file is compiled
    ROLLOUT_SHARDS + 1 times side by side (see "building in parallel" in it) and the objects are linked into libsumo_hip.so."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    inc = os.path.join(os.path.dirname(_CSRC), "..", "include")
    jobs = [
        ("libsumo_hip.so", "sumo_engine.hip", [["-DSUMO_ROLLOUT_EXTERN"]] + [["-DSUMO_ROLLOUT_SHARD=%d" % k] for k in range(ROLLOUT_SHARDS)]),
        ("libsumo_ppo.so", "ppo_kernels.hip", [[]]),
        ("libsumo_render.so", "sumo_render.hip", [[]]),
    ]
    out, links, compiles = [], [], []
    with tempfile.TemporaryDirectory(prefix="sumo_build_") as tmp:
        for target, src, units in jobs:
            src = os.path.join(_CSRC, src)
            if not os.path.exists(src):
                continue
            tpath = os.path.join(_CSRC, target)
            deps = [src] + [os.path.join(inc, h) for h in os.listdir(inc)] + [os.path.join(_CSRC, h) for h in os.listdir(_CSRC) if h.endswith(".h")]
            if force or _stale(tpath, deps):
                objs = [os.path.join(tmp, "%s.%d.o" % (target, k)) for k in range(len(units))]
                compiles += [[_hipcc(), "-O3", "-std=c++17", "--offload-arch=" + ARCH, "-fPIC", "-I", inc] + d + ["-c", src, "-o", o]
                             for d, o in zip(units, objs)]
                links.append((tpath, [_hipcc(), "-shared", "-fPIC", "-o", tpath] + objs))
            out.append(tpath)

        def run(cmd):
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)

        if compiles:
            with ThreadPoolExecutor(_workers()) as ex:
                list(ex.map(run, compiles))
        for tpath, cmd in links:
            run(cmd)
            _codegen_check(tpath)
    return out


def _codegen_check(lib):
    """After every (re)build: the static check for partial-EXEC save copies (codegen_check.py).  A hit does not stop the build -- the
    library is still the product and tests/test_codegen_check.py reports it -- unless SUMO_CODEGEN_CHECK=strict."""
    import sys
    try:
        from . import codegen_check
        hits = codegen_check.scan_library(lib)
    except Exception as e:                       # objcopy / llvm-objdump missing: the check is a development aid, not a build step
        print("codegen check skipped for %s: %r" % (os.path.basename(lib), e), file=sys.stderr)
        return
    if hits:
        msg = "%s: partial-EXEC save copies in %s (robosumo_selfplay_amd/codegen_check.py; perturb the source near them and rebuild)" % (
            os.path.basename(lib), ", ".join("%s x%d" % (k[:60], len(v)) for k, v in hits.items()))
        if os.environ.get("SUMO_CODEGEN_CHECK") == "strict":
            raise RuntimeError(msg)
        print("WARNING: " + msg, file=sys.stderr)


if __name__ == "__main__":
    print("\n".join(build_all(force=True, verbose=True)))
