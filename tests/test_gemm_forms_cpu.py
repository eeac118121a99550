"""CPU-only: the tile and 8-phase GEMM kernels in the built libicap_hip.so are exactly the recorded set.

tests/golden/gemm_kernel_forms.json holds the sorted names of every icap::gemm_kernel<...> and icap::gemm8p_kernel<...>
kernel, in gemm_plan_kernel_name's spelling, recorded from the library before the launchers were derived from
gemm_plan.h's table of forms (`python tests/test_gemm_forms_cpu.py` re-records it from the built library). A launcher
edit that adds, drops or changes an instantiation shows here, without a GPU."""
import json
import os
import pathlib
import re
import subprocess
import sys
import tempfile

from test_isa_cpu import OBJDUMP, _code_objects

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_kernel_forms.json")
SNAPSHOT = os.path.join(HERE, "golden", "gemm_plan_snapshot.json")

# a global function symbol of the code object's symbol table, demangled
_KERNEL = re.compile(r"^[0-9a-f]+ g\s+F \.text\s+[0-9a-f]+ (?:\.\w+ )?(?:void )?(icap::gemm(?:8p)?_kernel<.*>)\(icap_gemm_args,", re.M)


def _kernel_forms(objs):
    names = set()
    for o in objs:
        syms = subprocess.run([OBJDUMP, "-t", "-C", str(o)], check=True, capture_output=True, text=True).stdout
        for name in _KERNEL.findall(syms):
            # gemm_plan_kernel_name leaves the last template argument (ROLES) out where it is false
            if name.startswith("icap::gemm_kernel<"):
                assert name.count(",") == 10, name
                name = re.sub(r", false>$", ">", name)
            names.add(name)
    return sorted(names)


def test_kernel_set_is_the_recorded_one(tmp_path):
    built = _kernel_forms(_code_objects(tmp_path))
    golden = json.load(open(GOLDEN))
    assert golden == sorted(set(golden)) and len(golden) > 100
    assert built == golden, {"missing": sorted(set(golden) - set(built)), "new": sorted(set(built) - set(golden))}


def test_every_planned_kernel_is_built(tmp_path):
    """Each tile or 8-phase kernel name of the plan snapshot (tests/golden/gemm_plan_snapshot.json) is in the library."""
    built = set(_kernel_forms(_code_objects(tmp_path)))
    planned = [n for n in json.load(open(SNAPSHOT))["names"] if n.startswith(("icap::gemm_kernel<", "icap::gemm8p_kernel<"))]
    assert len(planned) > 20
    assert not [n for n in planned if n not in built]


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        forms = _kernel_forms(_code_objects(pathlib.Path(d)))
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(n) for n in forms) + "\n]\n")
    print(f"{out}: {len(forms)} kernels")
