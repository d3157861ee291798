"""include/usearch/index_dense.hpp — the reference's own class surface, `unum::usearch::index_dense_gt`, over the engine: compiles and
links everywhere, runs the reference's loops on an MI355X."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- include/usearch/index_dense.hpp: the reference's own class surface, `unum::usearch::index_dense_gt`, over the engine
CLASS_DIR = os.path.join(ROOT, "oracle", "_ref", "class")


def runnable_copy(binary: str, directory) -> str:
    """`binary` itself, or a copy of it in `directory` that names the libraries it needs by their file names. oracle/_ref is linked
    where the reference is mounted and run where the tree is copied to; a recipe that linked c/test.c against the class library by
    path recorded that path (DT_NEEDED), which does not exist there. The copy differs in those strings alone: each keeps its offset in
    the string table and ends earlier, and the loader finds the library through `class_environment()`."""
    entries = subprocess.check_output(["readelf", "-d", binary]).decode()
    by_path = [name for name in re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", entries) if "/" in name]
    if not by_path:
        return binary
    image = bytearray(open(binary, "rb").read())
    for path in by_path:
        recorded = path.encode() + b"\0"
        assert image.count(recorded) == 1, path
        at = image.index(recorded)
        name = os.path.basename(path).encode() + b"\0"
        image[at:at + len(name)] = name
    copy = os.path.join(directory, os.path.basename(binary))
    with open(copy, "wb") as out:
        out.write(image)
    os.chmod(copy, 0o755)
    return copy


def class_environment() -> dict:
    """The class library and the drop-in it leans on, first on the loader's search path."""
    search = [CLASS_DIR, os.path.join(ROOT, "usearch_amd", "lib")]
    if os.environ.get("LD_LIBRARY_PATH"):
        search.append(os.environ["LD_LIBRARY_PATH"])
    return dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(search))


def build_loop(directory) -> str:
    lib = os.path.join(ROOT, "usearch_amd", "lib")
    binary = os.path.join(directory, "usearch_amd_bench_loop")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bench_loop.cpp"), "-L", lib, "-l:libusearch_c.so",
                           f"-Wl,-rpath,{lib}", "-o", binary])
    return binary


def test_reference_shaped_caller_compiles_against_the_class_surface(tmp_path):
    """cpp/bench.cpp's add / search loops over `unum::usearch::index_dense_t` from include/usearch/index_dense.hpp."""
    binary = build_loop(tmp_path)
    assert "behind index_dense_t" in subprocess.check_output([binary, "link"]).decode()


def test_the_references_c_binding_compiled_against_the_class_surface_exports_the_abi(tmp_path):
    """oracle/Makefile `class_lib`: /root/reference/c/lib.cpp with `<usearch/index_dense.hpp>` resolving to THIS repository's
    header. The library must carry the reference's 38 symbols, defined by the reference's binding code, and lean on the drop-in."""
    library = os.path.join(CLASS_DIR, "libusearch_c_over_class.so")
    if not os.path.exists(library):
        pytest.skip("oracle/_ref/class was not built (`make -C oracle class_lib` needs /root/reference)")
    symbols = subprocess.check_output(["nm", "-D", "--defined-only", library]).decode()
    exported = {line.split()[-1] for line in symbols.splitlines() if " T usearch_" in line}
    assert len(exported) == 38 and {"usearch_init", "usearch_search", "usearch_filtered_search", "usearch_exact_search"} <= exported
    needed = subprocess.check_output(["readelf", "-d", library]).decode()
    assert "libusearch_c.so" in needed, "the class surface must reach the engine through the drop-in library"
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", library]).decode()
    assert "usearch_amd_c_api" in undefined
    # c/test.c linked against it finds every library it needs, wherever oracle/_ref was linked
    test_program = runnable_copy(os.path.join(CLASS_DIR, "reference_test_c"), tmp_path)
    loads = subprocess.run(["ldd", test_program], capture_output=True, text=True, env=class_environment())
    assert loads.returncode == 0 and "not found" not in loads.stdout, loads.stdout + loads.stderr
    assert os.path.join(CLASS_DIR, "libusearch_c_over_class.so") in loads.stdout, loads.stdout


@pytest.mark.gpu
def test_bench_loop_on_the_device(tmp_path):
    binary = build_loop(tmp_path)
    out = subprocess.run([binary, "run", str(tmp_path / "bench_loop.usearch")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "bench loop passed" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_the_references_own_c_test_passes_through_its_own_binding_over_the_class_surface(tmp_path):
    """/root/reference/c/test.c → (the reference's c/lib.cpp compiled against include/usearch/index_dense.hpp) → drop-in → MI355X."""
    binary = os.path.join(CLASS_DIR, "reference_test_c")
    if not os.path.exists(binary):
        pytest.skip("oracle/_ref/class was not built (`make -C oracle class_lib` needs /root/reference)")
    binary = runnable_copy(binary, tmp_path)
    # (c/test.c saves and views "tmp.usearch" in its working directory)
    result = subprocess.run([binary], capture_output=True, text=True, timeout=900, env=class_environment(), cwd=tmp_path)
    assert result.returncode == 0, result.stdout[-3000:] + result.stderr[-3000:]
