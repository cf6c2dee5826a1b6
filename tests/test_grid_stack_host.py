"""The tiling and the block / thread decode of csrc/grid_stack.h -- what gq_clutter_compose_kernel, gq_tsdf_integrate_kernel and
the surfel kernels run to find their node -- compiled for the HOST with AddressSanitizer and UBSan and run as a program of its own
(tests/grid_stack_host.cpp): every block x 256 threads of a launch is walked, every node of every grid must be given to exactly one
thread, no thread beyond a partial tile may pass the bounds test, and no block may name a grid the stack does not have.  The marks
live in one allocation of exactly nx ny nz bytes per grid, so a node outside the grid ends the program.  No GPU involved."""
import subprocess

import pytest

import _host_program

SHAPES = [(2, 2, 2),  # the smallest legal grid
          (4, 4, 16),  # exactly one full tile
          (5, 9, 17), (9, 8, 17),  # partial tiles on every axis: the layouts of the GPU tests
          (17, 5, 33)]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = _host_program.build("grid_stack_host", tmp_path_factory.mktemp("grid_stack"))
    return lambda G, shape: int(subprocess.check_output([exe, str(G), *map(str, shape)]))  # a non-zero exit raises


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_node_of_every_grid_is_one_thread_of_one_block(walk, shape, G):
    nx, ny, nz = shape
    assert walk(G, shape) == G * ((nx + 3) // 4) * ((ny + 3) // 4) * ((nz + 15) // 16)
