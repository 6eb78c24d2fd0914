"""CPU: timeline training on the lane-array build of the kernel sources (tests/emu) -- scanc_unit's checkpointing form, scanp_bwd_wave and
convp_bwd_wave run as host code through aum_scan_tm_peeks_fwd_ckpt / aum_scan_tm_peeks_bwd / aum_conv1d_tm_peeks_bwd, the bindings, the
autograd functions, Mamba.forward(peek_every=) and AudioMamba.forward_timeline (tests/timeline_train_checks.py).  The device kernels are
held to the same checks in tests/test_gpu_timeline_train.py.
On the commit before the feature every test here fails: the library has no aum_*_tm_peeks_* symbols, aum_hip no *_tm_peeks_* functions,
the interfaces no *_peeks_fn / *_peeks_ref, `peek_every=` is no argument of Mamba.forward and AudioMamba has no forward_timeline."""
import os
import sys

import pytest
import torch

import aum_hip
import timeline_train_checks as tt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build_emu
    return aum_hip.Lib(build_emu.build(), host=True)


@pytest.fixture()
def emu_as_product(lib):
    old = aum_hip._product
    aum_hip._product = lib
    yield
    aum_hip._product = old


def test_names_are_declared_and_exported(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aum_hip.h")).read()
    for name in ("aum_scan_tm_peeks_fwd_ckpt", "aum_scan_tm_peeks_bwd", "aum_conv1d_tm_peeks_bwd"):
        assert f"int {name}(" in header and name in aum_hip.EXPORTS and hasattr(lib.c, name)
    assert aum_hip.ABI_VERSION == 13 and lib.c.aum_abi_version() == 13
    assert lib.c.aum_scan_tm_peeks_ckpt_bytes(27, 2, 128, 16) == (27 // 8 + 2) * 128 * 16 * 4
    assert lib.c.aum_scan_tm_peeks_bwd_workspace_bytes(27, 2, 128, 16) == (2 * 27 * 32 + 2 * 128 * 18) * 4
    assert lib.c.aum_conv1d_tm_peeks_bwd_workspace_bytes(2, 128, 4) == 2 * 128 * 5 * 4


def test_struct_layouts_match_the_header(tmp_path):
    import ctypes
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probes = {"AumScanTmPeeksFwdArgs": (aum_hip.ScanTmPeeksFwdArgs, ["base", "ckpt", "ckpt_bytes", "peek_every"]),
              "AumScanTmPeeksBwdArgs": (aum_hip.ScanTmPeeksBwdArgs, ["base", "ckpt", "du", "ddelta", "dz", "workspace", "ckpt_bytes", "workspace_bytes",
                                                                    "du_ts", "ddelta_ts", "dz_ts", "peek_every"]),
              "AumConvTmPeeksBwdArgs": (aum_hip.ConvTmPeeksBwdArgs, ["x", "dy", "weight", "bias", "dx", "workspace", "cu_seqlens", "workspace_bytes", "x_ts",
                                                                    "dy_ts", "dx_ts", "total", "nseq", "dim", "width", "dtype", "flags", "peek_every"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(root, "include", "aum_hip.h")}"', "int main(void){"]
    for cname, (_, fields) in probes.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, (cls, fields) in probes.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def _kind(P, dim):
    return tt.PERIODS.index(P) + tt.DIMS.index(dim)


@pytest.mark.parametrize("P", tt.PERIODS)
@pytest.mark.parametrize("dim", tt.DIMS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_forward_is_the_inference_kernel_on_a_zeroed_pool(dt, dim, P, lib):
    tt.check_forward_identity(dt, dim, P, lib, "cpu", kind=_kind(P, dim))


@pytest.mark.parametrize("P", tt.PERIODS)
@pytest.mark.parametrize("dim", tt.DIMS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_gradients_against_float64(op, dt, dim, P, lib):
    tt.check_gradients(op, dt, dim, P, lib, "cpu", kind=_kind(P, dim))


@pytest.mark.parametrize("P", tt.PERIODS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_peek_rows_do_not_leak(op, dt, P, lib):
    dim = tt.DIMS[tt.PERIODS.index(P) % 2]
    tt.check_peek_rows_do_not_leak(op, dt, dim, P, lib, "cpu", kind=_kind(P, dim) + 1)


@pytest.mark.parametrize("P", tt.PERIODS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("op", ["conv", "scan"])
def test_repeatable_and_independent_of_the_pack(op, dt, P, lib):
    dim = tt.DIMS[(tt.PERIODS.index(P) + 1) % 2]
    tt.check_repeatable_and_isolated(op, dt, dim, P, lib, "cpu", kind=_kind(P, dim) + 2)


def test_refusals_touch_nothing(lib):
    tt.check_refusals(lib, "cpu")


@pytest.mark.parametrize("d_model", [64, 192])
def test_module_matches_its_ref_twin(d_model, emu_as_product):
    tt.check_module(d_model, "cpu")


@pytest.mark.parametrize("embed_dim", [64, 192])
def test_model_forward_timeline(embed_dim, emu_as_product):
    tt.check_model(embed_dim, "cpu")


def test_model_refuses_non_streamable_configurations(emu_as_product):
    tt.check_model_refuses_non_streamable("cpu")


def test_model_forward_timeline_from_a_waveform(emu_as_product):
    tt.check_model_frontend("cpu")


def test_launcher_timeline_loss(tmp_path, emu_as_product):
    """through the lane-array library (no _ref twins needed: a tiny one-block model on four columns takes about a second)"""
    tt.check_launcher(tmp_path)
