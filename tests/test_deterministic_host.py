"""CPU checks of the deterministic training mode: the C entry point, the instruction stream of the built library (the mode's kernel
variants hold no float atomic; the only kernels that do are the six default-mode reductions the mode replaces), the seeded initial
weights and train.py --deterministic."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scann_hip.h")

FLOAT_ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic_(add_f32|pk_add_\w+)\b|\bds_(pk_)?add_(rtn_)?\w*f32\b|\bds_pk_add_\w+\b")
# the six reductions of the 128-wide backward that end in float atomics in the default mode, and their deterministic variants
DEFAULT_ATOMIC = {"readout_bwd_kernel", "basis_bwd_kernel", "base_geom_bwd_kernel", "embed_scatter_kernel", "embed_bwd_kernel",
                  "embed_general_bwd_kernel"}
DET_VARIANTS = {"readout_bwd_det_kernel", "basis_bwd_det_kernel", "base_geom_bwd_det_kernel", "embed_scatter_det_kernel",
                "embed_bwd_det_kernel", "embed_general_bwd_det_kernel", "scalar_sum_kernel"}


def test_set_deterministic_is_declared_and_exported(hip_lib):
    from scann import _hip

    src = open(HEADER).read()
    assert re.search(r"int\s+scann_set_deterministic\s*\(\s*scann_handle_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", src)
    assert re.search(r"#define\s+SCANN_ABI_VERSION\s+1\b", src)
    assert hasattr(_hip.load_library(), "scann_set_deterministic")
    assert "scann_set_deterministic" in [n for n, _, _ in _hip.SYMBOLS]


def _kernel_isa(so_path):
    """{demangled-ish kernel name (the scann:: function name): set of float-atomic mnemonics} over every gfx950 code object of the
    library (the .hip_fatbin bundles, extracted as test_host._device_kernels does), from llvm-objdump -d"""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM binutils not found")
    tmp = tempfile.mkdtemp(prefix="scann_det_")
    try:
        fat = os.path.join(tmp, "fatbin")
        subprocess.check_call([tools[0], "--dump-section", ".hip_fatbin=" + fat, so_path])
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
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--output=" + co])
            cur = None
            for line in subprocess.check_output([tools[2], "-d", co], text=True).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    sym = m.group(1)
                    mm = re.match(r"_ZN5scann(\d+)", sym)
                    cur = sym[len(mm.group(0)):len(mm.group(0)) + int(mm.group(1))] if mm else sym
                    out.setdefault(cur, set())
                    continue
                if cur is not None:
                    f = FLOAT_ATOMIC.search(line)
                    if f:
                        out[cur].add(f.group(0))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_deterministic_kernels_have_no_float_atomics(hip_lib):
    from scann import _hip

    isa = _kernel_isa(_hip.LIB_PATH)
    missing = DET_VARIANTS - set(isa)
    assert not missing, missing
    for name in DET_VARIANTS:
        assert not isa[name], (name, isa[name])
    # regression guard: exactly the six default-mode reductions hold float atomics, nothing else in the library
    assert {k for k, v in isa.items() if v} == DEFAULT_ATOMIC, {k: v for k, v in isa.items() if v}


def test_deterministic_config_seeds_the_initial_weights(hip_lib):
    from scann.models.scann_model import keras_default_init, normalize_config

    import scann_oracle as so

    cfg = normalize_config(so.default_config("qm9"))
    assert cfg["hyper"]["deterministic"] is False
    cfg["hyper"].update(deterministic=True, seed=7)
    specs = so.weight_shapes(cfg)
    a = keras_default_init(specs, cfg["hyper"]["seed"])
    b = keras_default_init(specs, cfg["hyper"]["seed"])
    c = keras_default_init(specs, 8)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert any(not np.array_equal(a[k], c[k]) for k in a if a[k].std() > 0)


def test_scann_facade_draws_the_weights_from_hyper_seed(monkeypatch):
    """SCANN(config) passes hyper.seed to create_model when hyper.deterministic is set, and keeps the unseeded call otherwise"""
    from scann.models import scann_model

    seen = []
    monkeypatch.setattr(scann_model, "create_model", lambda config, seed=None: seen.append(seed) or "model")
    scann_model.SCANN({"model": {}, "hyper": {"deterministic": True, "seed": 7}})
    scann_model.SCANN({"model": {}, "hyper": {"deterministic": True}})
    scann_model.SCANN({"model": {}, "hyper": {}})
    assert seen == [7, 0, None]


def test_train_cli_deterministic_reaches_the_config(tmp_path):
    import yaml

    spec = importlib.util.spec_from_file_location("train_cli_det", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = {"model": {"feature": "x", "use_ring": None, "use_drop": None}, "hyper": {"target": None, "pretrained": None, "use_ref": None}}
    path = tmp_path / "d.yaml"
    path.write_text(yaml.safe_dump(cfg))
    a = cli.parser().parse_args(["homo", str(path), "--seed", "7", "--deterministic", "True"])
    assert a.deterministic is True
    c = cli.configured(a)
    assert c["hyper"]["deterministic"] is True and c["hyper"]["seed"] == 7
    a = cli.parser().parse_args(["homo", str(path)])
    assert a.deterministic is False
    assert "deterministic" not in cli.configured(a)["hyper"]
