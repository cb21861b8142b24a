"""Build a variant of libmaple_hip_debug.so (the product units plus the unit of include/maple_hip_debug.h, all with the extra flags)
next to the product library: tools/build_variant.py NAME [extra hipcc flags ...]
-> maple_amd/libmaple_hip_NAME.so (objects under build/NAME/).  Run anything with MAPLE_HIP_LIB=<that path> to use it
(tools that open Device(debug=True): MAPLE_HIP_LIB_DEBUG=<that path> as well -- runtime.load_library keeps the two apart)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
name, extra = sys.argv[1], sys.argv[2:]
out = os.path.join(ROOT, "build", name)
os.makedirs(out, exist_ok=True)
lib = os.path.join(ROOT, "maple_amd", f"libmaple_hip_{name}.so")
g.link(lib, g.compile_units(out, extra))
print(lib)
