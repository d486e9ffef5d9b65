"""The chunk arithmetic of the row uploads (vsc2022_amd/csrc/row_chunks.h) on the CPU: tests/row_chunks_main.cpp, a
stand-alone program over that header alone, built with the host compiler under the address and undefined-behaviour
sanitizers.  The walk it checks is the loop of `for_row_chunks` (api_internal.h), which every upload of rows goes through;
no GPU test reaches the second chunk of the 256 MB paths.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_pieces_cover_source_and_output_rows_once(tmp_path):
    cxx = os.environ.get("CXX") or next(c for c in ("c++", "g++", "clang++") if shutil.which(c))
    exe = str(tmp_path / "row_chunks_main")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "vsc2022_amd", "csrc"),
                            os.path.join(ROOT, "tests", "row_chunks_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "row_chunks ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
