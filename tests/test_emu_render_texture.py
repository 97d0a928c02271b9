"""The textured albedo of the template rasteriser (csrc/s6d_raster.hip) executed on the HOST through the emulated HIP runtime: the
bodies of tests/test_gpu_render_texture.py at the same shapes (the kernel source itself runs: the pyramid kernel, the resolve kernel's
texture policy with the level rule, the wrap and the bilinear sample)."""
import pytest

from tests import test_gpu_render_texture as T


@pytest.mark.parametrize("shape", [(3, 5), (7, 1), (8, 8), (32, 64)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_pyramid_on_the_emulator(emu, shape):
    T.check_pyramid(emu, shape)


def test_quad_level_0_on_the_emulator(emu):
    T.check_quad(emu)


def test_wrap_on_the_emulator(emu):
    T.check_wrap(emu)


def test_minification_on_the_emulator(emu):
    T.check_minified(emu)


def test_odd_sizes_on_the_emulator(emu):
    T.check_odd(emu)


@pytest.mark.parametrize("name", ["cube", "torus"])
def test_mesh_vs_restatement_on_the_emulator(emu, name):
    T.check_mesh(emu, name)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e30], ids=["nan", "inf", "1e30"])
def test_hostile_uv_on_the_emulator(emu, value):
    T.check_hostile(emu, value)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)


def test_render_templates_textured_on_the_emulator(emu):
    T.check_render_templates(emu)
