"""TEST INFRASTRUCTURE ONLY.  Compiles the reference's own C++ example programs against the facade
(include/ggnn/base/ggnn.cuh) from where they lie in the reference tree and records the outcome in
oracle/_ref/examples/<name>.json for tests/test_cpp_facade.py.  Run by `make -C oracle ref`, only
where the reference tree is available; nothing of the examples is written anywhere (the one edited
source goes to the compiler on stdin).

    python ref_examples.py <reference tree> <out dir>

ggnn_main.cpp, ggnn_main_multi_gpu.cpp: compiled unchanged.
ggnn_main_gpu_data.cu (the caller that hands the engine data living on the GPU): its ggnn lines
(47-65: setBase(referenceGPUData), the GPU query dataset, build, query, structured bindings) are
compiled UNCHANGED; the CUDA runtime calls around them are renamed to HIP and the cuRAND fill is
dropped, textually (SURVEY section 7-2 allows exactly that)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++20", "-O2", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT}/include", "-I/opt/rocm/include"]
EXAMPLES = "examples/cpp-and-cuda"


def gpu_data_source(path):
    """the example with its CUDA runtime calls swapped for HIP; raises if its ggnn lines are not
    where and what the test expects, or would be touched"""
    lines = open(path).read().splitlines()
    body = lines[46:65]
    assert any("referenceGPUData(base, N_base, D, gpu_id)" in l for l in body), "setBase line"
    assert any("ggnn.query(d_query, KQuery" in l for l in body), "query line"
    out = []
    for n, l in enumerate(lines):
        if "curand" in l:
            assert not 46 <= n < 65, "cuRAND inside the ggnn lines"
            continue
        if not 46 <= n < 65:
            l = (l.replace("#include <cuda_runtime.h>", "#include <hip/hip_runtime_api.h>")
                  .replace("cudaMalloc(", "(void)hipMalloc(").replace("cudaFree(", "(void)hipFree("))
        out.append(l)
    assert out[out.index(body[0]):][:len(body)] == body, "the ggnn lines changed"
    return "\n".join(out) + "\n"


def compile_one(name, ref, out_dir):
    path = os.path.join(ref, EXAMPLES, name)
    obj = os.path.join(out_dir, os.path.splitext(name)[0] + ".o")
    result = {"example": f"{EXAMPLES}/{name}", "edited": name.endswith(".cu")}
    try:
        if result["edited"]:
            src = gpu_data_source(path)
            cmd = ["g++", *FLAGS, "-x", "c++", "-c", "-", "-o", obj]
        else:
            src = None
            cmd = ["g++", *FLAGS, "-c", path, "-o", obj]
        r = subprocess.run(cmd, input=src, capture_output=True, text=True)
        result.update(returncode=r.returncode, log=(r.stdout + r.stderr)[-4000:])
    except (AssertionError, OSError) as e:
        result.update(returncode=None, log=f"{type(e).__name__}: {e}")
    with open(os.path.join(out_dir, os.path.splitext(name)[0] + ".json"), "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    ref, out_dir = sys.argv[1], sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    for name in ("ggnn_main.cpp", "ggnn_main_multi_gpu.cpp", "ggnn_main_gpu_data.cu"):
        compile_one(name, ref, out_dir)
