"""Host builds of the DEVICE sources that more than one test module needs (plain helpers, no fixtures): the scaffold
of csrc/mpe_ddmath.h (tests/host/ddmath_host.cpp) and of the geometry (tests/host/geom_host.cpp), compiled through
tests/host/stub.  tests/test_ddmath_host.py and tests/test_geometry_host.py build them for the CPU tier,
tests/test_ddmath_device.py builds the same two to hold the amdgcn build of the same source to their bits."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rpg_monocular_pose_estimator_amd", "csrc")
# the reference build of the CPU tier: no a * b + c fusion, as the device build (csrc/Makefile)
GXX = ("g++", "-O1", "-ffp-contract=off")


def rocm_clangxx():
    """ROCm's clang++ (the front end and optimiser the device build goes through), or None."""
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        for rel in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
            p = os.path.join(root or "", rel)
            if root and os.path.exists(p):
                return p
    return None


def _env_flags():
    return os.environ.get("MPE_HOST_CXXFLAGS", "").split()


def build_ddmath_host(d, compiler=GXX, name="libddm_host.so"):
    """tests/host/ddmath_host.cpp -> a shared library in directory d.  compiler: the command and its optimisation /
    contraction flags."""
    so = os.path.join(str(d), name)
    subprocess.check_call([*compiler, "-std=c++17", "-shared", "-fPIC", *_env_flags(), "-w",
                           "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "ddmath_host.cpp"), "-o", so])
    return C.CDLL(so)


def build_geom_host(d):
    """tests/host/geom_host.cpp (mpe_p3p.h as it is, the tail helpers of mpe_k3.hip and the index arithmetic of
    mpe_k2.hip cut out of the kernel text) -> a shared library in directory d."""
    import rpg_monocular_pose_estimator_amd as mpe
    hip = mpe.device_source()
    i = hip.index("struct T34 {")
    with open(os.path.join(d, "k3_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("#define K3_GROUP", i)])
    i = hip.index("// lexicographic unranking of the idx-th 3-combination")
    with open(os.path.join(d, "k2_extract.inc"), "w") as fh:
        fh.write(hip[i:hip.index("#define K2_THREADS", i)])
        i = hip.index("__device__ __forceinline__ void perm_from_index(")
        fh.write(hip[i:hip.index("// one entry of the table (layout above) -> e", i)])
    so = os.path.join(d, "libgeom_host.so")
    subprocess.check_call([*GXX, "-std=c++17", "-shared", "-fPIC", *_env_flags(), "-I", str(d),
                           "-I", os.path.join(ROOT, "tests", "host", "stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "geom_host.cpp"), "-o", so])
    return C.CDLL(so)
