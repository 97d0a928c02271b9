"""The template rasteriser (csrc/s6d_raster.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_render.py at the same shapes (the kernel source itself runs: the float32 vertex stage, the integer coverage rule,
both work shapes and the list between them, the 64-bit minimum, the resolve stage)."""
import pytest

from tests import test_gpu_render as T


@pytest.mark.parametrize("name", ["torus", "cube", "cube-near"])
def test_mesh_vs_restatement_on_the_emulator(emu, name):
    T.check_mesh(emu, name)


def test_fill_rule_on_the_emulator(emu):
    T.check_fill_rule(emu)


@pytest.mark.parametrize("name", sorted(T.HOSTILE))
def test_hostile_geometry_on_the_emulator(emu, name):
    T.check_hostile(emu, name)


def test_determinism_on_the_emulator(emu):
    T.check_determinism(emu)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)


def test_render_templates_layout_on_the_emulator(emu):
    T.test_render_templates_layout(emu)
