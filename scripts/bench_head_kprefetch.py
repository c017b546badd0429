"""Development aid: bench.py's own timed loop with RPSF_OPT_HEAD_KPREFETCH pinned on every plan it creates (bench.py itself is not touched).
    python scripts/bench_head_kprefetch.py 0|1 [bench.py arguments]"""
import pathlib
import runpy
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from regularizepsf_amd import _native  # noqa: E402

value = int(sys.argv[1])
plan_init = _native.Plan.__init__


def init(self, *args, **kwargs):
    plan_init(self, *args, **kwargs)
    self.set_option("head_kprefetch", value)  # (ignored by plans other than 256-pixel ones)


_native.Plan.__init__ = init
sys.argv = [str(ROOT / "bench.py"), *sys.argv[2:]]
runpy.run_path(str(ROOT / "bench.py"), run_name="__main__")
