"""Sharding by index mod world from the compiled hosts: the C++ mirror (tests/cpp/test_shard_layout.cpp over zk_amd/host/zk.hpp,
built here into a temporary directory with the flags of tests/cpp/Makefile) and the Rust shim's safe wrappers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_shard_layout.cpp")
SHIM = os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")


def _build(tmp_path):
    exe = str(tmp_path / "test_shard_layout")
    lib_dir = os.path.join(ROOT, "zk_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, SRC, "-L" + lib_dir, "-lzk_amd", "-Wl,-rpath," + lib_dir],
                   check=True, capture_output=True, text=True)
    return exe


def test_cpp_shard_layout_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    exe = _build(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no CPU fallback" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_shard_layout_on_gpu(tmp_path):
    """new_shard / split / interleave through zk.hpp, checked by the program itself against its host table"""
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: shard layout host tests passed" in r.stdout


def _method(src, name):
    """body of `pub fn name(` inside the shim (up to the next `pub fn` or the end of the impl)"""
    m = re.search(r"pub fn " + name + r"\b(.*?)(?=\n    /// |\n    pub fn |\n}\n)", src, flags=re.S)
    assert m, f"MultiLinearPolynomial::{name} is missing from the Rust shim"
    return m.group(1)


def test_rust_shim_has_safe_shard_wrappers():
    src = open(SHIM).read()
    impl = src[src.index("impl<F: GpuField> MultiLinearPolynomial<F> {"):]
    new_shard = _method(impl, "new_shard")
    assert re.match(r"\(n_vars: usize, evaluations: &\[F\], world: u32, rank: u32\) -> Result<Self, &'static str>", new_shard)
    assert "zk_mle_upload_shard(" in new_shard
    split = _method(impl, "split")
    assert re.match(r"\(&self, world: u32\) -> Result<Vec<Self>, &'static str>", split)
    assert "zk_mle_split(" in split
    inter = _method(impl, "interleave")
    assert re.match(r"\(shards: &\[Self\]\) -> Result<Self, &'static str>", inter)
    assert "zk_mle_interleave(" in inter
    assert "fn zk_mle_unshard" not in src   # needs a communicator type the shim does not have
