"""CPU: shardplan::update_blocks (csrc/shard_plan.h), the byte offsets of the scratch blocks of vidc_shards_translate_labels_dev,
vidc_sharded_append_dev and vidc_remove_sharded_dev -- the home block and the block of a shard on another device, whose staging has
never run on a GPU.  tests/shard_blocks_test.cpp walks 4 shard counts x 6 request counts x 16 combinations of optional sections x
(no masks + 6 sets of mask lengths) and asserts alignment, disjointness and sizes; built with g++ as a stand-alone program, once more
under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = 4 * 6 * 16 * 7


@pytest.mark.parametrize("sanitize", [False, True])
def test_shard_blocks_program(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "shard_blocks_test")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "shard_blocks_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and f"shard blocks ok: {LAYOUTS} layouts" in out.stdout, out.stdout + out.stderr
