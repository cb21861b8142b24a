"""A variant of the product library in which only SOME translation units are compiled with extra flags (the others are the objects
of the regular build): tools/build_unit_variant.py NAME unit.hip[,unit2.hip] [extra hipcc flags ...]
-> maple_amd/libmaple_hip_NAME.so.  Run anything with MAPLE_HIP_LIB=<that path> to use it."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
name, units, extra = sys.argv[1], sys.argv[2].split(","), sys.argv[3:]
out = os.path.join(ROOT, "build", name)
os.makedirs(out, exist_ok=True)
lib = os.path.join(ROOT, "maple_amd", f"libmaple_hip_{name}.so")
g.link(lib, g.compile_units(out, extra, only=units)[:-1])
print(lib)
