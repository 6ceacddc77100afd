"""oracle/needed.py: a binary linked against libmulls_hip.so by path (the library has no SONAME, so the path is what DT_NEEDED records) is made to
load it by name, through its $ORIGIN run path, from whichever checkout it sits in — what build() does to an oracle/_ref/adapter_check built elsewhere."""
import os
import shutil
import subprocess

import pytest

from oracle import needed


def _needed(path):
    out = subprocess.check_output(["readelf", "-d", path], text=True)
    return [l.split("[", 1)[1].rstrip("]") for l in out.splitlines() if "(NEEDED)" in l]


def test_path_entry_becomes_the_bare_name_and_resolves_in_the_new_checkout(tmp_path):
    if shutil.which("gcc") is None or shutil.which("readelf") is None:
        pytest.skip("needs gcc and readelf")
    built = tmp_path / "built"  # the checkout the binary was linked in
    (built / "mulls_amd").mkdir(parents=True)
    (built / "oracle" / "_ref").mkdir(parents=True)
    (tmp_path / "lib.c").write_text("int mulls_probe(void) { return 42; }\n")
    (tmp_path / "main.c").write_text("int mulls_probe(void);\nint main(void) { return mulls_probe() == 42 ? 0 : 1; }\n")
    lib = built / "mulls_amd" / "libmulls_hip.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(lib), str(tmp_path / "lib.c")])
    exe = built / "oracle" / "_ref" / "adapter_check"
    subprocess.check_call(["gcc", "-o", str(exe), str(tmp_path / "main.c"), str(built / "oracle" / ".." / "mulls_amd" / "libmulls_hip.so"),
                           "-Wl,-rpath,$ORIGIN/../../mulls_amd"])
    assert _needed(str(exe))[0] == str(built / "oracle" / ".." / "mulls_amd" / "libmulls_hip.so")

    moved = tmp_path / "moved"  # another checkout: the library of the first one is gone
    shutil.copytree(built, moved)
    shutil.rmtree(built)
    exe2 = moved / "oracle" / "_ref" / "adapter_check"
    assert subprocess.run([str(exe2)], capture_output=True).returncode == 127  # the recorded path does not exist any more
    mode = os.stat(exe2).st_mode
    assert needed.by_name(str(exe2))
    assert _needed(str(exe2))[0] == "libmulls_hip.so" and os.stat(exe2).st_mode == mode
    assert subprocess.run([str(exe2)]).returncode == 0  # found through $ORIGIN in the new checkout
    assert not needed.by_name(str(exe2))  # a second pass changes nothing
    assert sorted(os.listdir(exe2.parent)) == ["adapter_check"]
