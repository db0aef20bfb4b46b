"""The deciding half of the Elias-Fano host calls (csrc/ef_plan.h): geometry, tiling, chunk-kernel form, clearing, records, decode
form, the speculative stream bounds and the sort plan, built with g++ (no HIP, no GPU); and the tie between ef_chunk_form, which the
library runs, and lists_ref.encoder_form, the restatement the GPU files select their objects by."""
import os
import shutil
import subprocess

import pytest

import lists_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("ef_plan") / "ef_plan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-o", path, os.path.join(ROOT, "tests", "ef_plan_test.cpp")])
    return path


def test_ef_plan(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ef plan ok" in out.stdout, out.stdout + out.stderr


def test_encoder_form_is_the_hosts_choice(exe):
    """every object of lists_ref.OBJECTS under the routes the single-pass encoder finishes: what ef_chunk_form answers for the
    figures the host call holds (lists, ids, 512-id chunks, longest list, any id of 2^32 or more) is lists_ref.encoder_form"""
    cases, lines = [], []
    for name in lr.OBJECTS:
        for route in ("host", "wide"):
            lists, _ = lr.object_lists(name, route)
            sizes = [len(li) for li in lists]
            nchunks = sum((n + lr.CHUNK - 1) // lr.CHUNK for n in sizes)
            wide = any(len(li) and int(li[-1]) >= lr.NARROW for li in lists)
            cases.append((name, route, lr.encoder_form(lists)))
            lines.append(f"{len(lists)} {sum(sizes)} {nchunks} {max(sizes)} {int(wide)}")
    out = subprocess.run([exe, "query"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split()
    assert len(got) == len(cases)
    for (name, route, want), form in zip(cases, got):
        assert form == want, (name, route, form, want)
    assert {w for _, _, w in cases} == {"short", "half", "full", "wide"}  # (the table reaches every form the host can choose)
