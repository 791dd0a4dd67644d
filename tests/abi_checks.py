"""What the host tests of the analyses share: the C header read once, the ctypes table checked against expected signatures, the kernel
descriptors of the built library read once, and the HipModel stand-in the Python-layer tests run on.  No GPU."""
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def header():
    """include/scann_hip.h with every run of white space made one blank"""
    return " ".join(open(os.path.join(ROOT, "include", "scann_hip.h")).read().split())


def declared(*texts):
    """every text stands in the (flattened) header"""
    flat = header()
    for text in texts:
        assert " ".join(text.split()) in flat, text


def signatures(want):
    """{name: (restype, argtypes)} is what _hip.SYMBOLS binds under those names"""
    from scann import _hip

    sig = {n: (r, a) for n, r, a in _hip.SYMBOLS}
    for name, (restype, argtypes) in want.items():
        assert name in sig, name
        assert sig[name] == (restype, list(argtypes)), (name, sig[name])
    return sig


_KERNELS = {}


def device_kernels(so_path):
    """{mangled kernel name: (scratch bytes per lane, VGPRs)} of every gfx950 code object inside a shared library: the .hip_fatbin
    section holds one clang offload bundle per .hip source file; their ELF notes carry the kernel descriptors' metadata.  One library
    (path, mtime, size) is taken apart once; a skip is not remembered."""
    st = os.stat(so_path)
    key = (os.path.abspath(so_path), st.st_mtime_ns, st.st_size)
    if key not in _KERNELS:
        _KERNELS[key] = _read_device_kernels(so_path)
    return _KERNELS[key]


def _read_device_kernels(so_path):
    import shutil
    import tempfile

    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM binutils not found")
    tmp = tempfile.mkdtemp(prefix="scann_co_")
    try:
        fat = os.path.join(tmp, "fatbin")
        # (with an output file: without one llvm-objcopy writes the library back in place, a new mtime on every call)
        subprocess.check_call([tools[0], "--dump-section", ".hip_fatbin=" + fat, so_path, os.path.join(tmp, "copy")])
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts, i = [], blob.find(magic)
        while i >= 0:
            starts.append(i)
            i = blob.find(magic, i + 1)
        out = {}
        for k, a in enumerate(starts):
            part, co = os.path.join(tmp, "b%d" % k), os.path.join(tmp, "c%d.co" % k)
            open(part, "wb").write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            name = scratch = None
            for line in subprocess.check_output([tools[2], "--notes", co], text=True).splitlines():
                line = line.strip()
                if line.startswith(".name:"):
                    name = line.split()[-1]
                elif line.startswith(".private_segment_fixed_size:"):
                    scratch = int(line.split()[-1])
                elif line.startswith(".vgpr_count:") and name is not None:
                    out[name] = (scratch, int(line.split()[-1]))
                    name = scratch = None
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def stand_in_model(cfg, engine, ring=False):
    """a HipModel that never saw a device: the normalised config, the input names (ring_aromatic among them if ``ring`` and the config
    uses it) and ``engine(config)`` as its engine"""
    from scann.models.scann_model import INPUT_NAMES, HipModel, normalize_config

    m = HipModel.__new__(HipModel)
    m.config = normalize_config(cfg)
    m.engine = engine(m.config)
    m.input_names = list(INPUT_NAMES) + (["ring_aromatic"] if ring and m.config["model"]["use_ring"] else [])
    return m
