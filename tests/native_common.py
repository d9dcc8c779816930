"""What the CPU test modules share about native code: the stand-alone C++ harnesses of tests/native/ (built with g++ and run as
programs of their own), the stand-in for a reference checkout behind compat/, and the C ABI of include/vfa_hip.h."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_VERSION = 9  # the one statement of the expected VFA_ABI_VERSION; an ABI change edits this line
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_harness(tmp_path_factory, name, source, flags, sanitized=False):
    """Compile ``tests/native/<source>`` with ``g++ <flags>`` into a fresh directory -> the program's path.  ``sanitized``: the
    same stand-alone program (its own ``main``, nothing preloaded) with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path_factory.mktemp(name + ("_san" if sanitized else "")) / "harness")
    subprocess.check_call(["g++", *flags, *(SANITIZE if sanitized else []), "-o", exe, os.path.join(REPO, "tests", "native", source)])
    return exe


def run_harness(exe, *args, timeout=300):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
    return out.stdout


def write_checkout(root, files):
    """A stand-in for the reference checkout behind compat/: ``files`` maps relative paths of the layout the alias package extends
    to module texts of a line or two, each test stating its own table -> the checkout's path."""
    for rel, text in files.items():
        path = root / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(text)
    return str(root)


def declared_parameters():
    """Every function include/vfa_hip.h declares (comments stripped) -> ``{name: number of parameters}``, ``(void)`` counting 0."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vfa_hip.h")).read(), flags=re.S)
    found = re.findall(r"\b(?:int|size_t)\s+(vfa_\w+)\s*\((.*?)\)\s*;", text, flags=re.S)
    return {name: 0 if args.strip() in ("", "void") else len(args.split(",")) for name, args in found}
