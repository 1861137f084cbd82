"""The grid of a k_shade launch and its switch (csrc/kernels.h shade_grid_blocks, csrc/settings.h XRT_SHADE_BLOCK) on the host.  The program
tests/shade_blocks/host_shade_blocks.cpp, built with host ASan + UBSan (csrc/Makefile `hostcheck_shade_blocks`), checks for every block size from 256 to 1024
that an unknown generation gets the fewest blocks that hold 2^20 threads (1024 x 1024 and 4096 x 256, the grids the two fixed sizes had), that a hint in rays
gives a thread per ray up to that cap and no block more, for ray counts around the block size, the small-generation threshold and 2^31; and that the switch
takes 256 .. 1024 in steps of 64 and leaves the default for anything else.  The frames themselves: tests/test_gpu_shade_blocks.py."""
import os
import re
import subprocess

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")


def test_grid_and_switch_of_every_block_size():
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_shade_blocks"])
    env = {k: v for k, v in os.environ.items() if k != "XRT_SHADE_BLOCK"}
    p = subprocess.run([os.path.join(CSRC, "hostcheck_shade_blocks")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "host_shade_blocks: ok" in p.stdout
    assert int(re.search(r"^default (\d+)$", p.stdout, flags=re.M).group(1)) == 768   # two blocks per CU (profiles/shade_blocks)
