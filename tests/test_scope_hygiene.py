"""The oracle is test infrastructure: nothing in the product package (or tools/) may import it, and the
product must not fall back to it.  bench.py may only touch it inside cpu_baseline(); __graft_entry__ only
inside smoke()."""
import ast
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _imports_oracle(path):
    tree = ast.parse(open(path).read())
    hits = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            hits += [n.name for n in node.names if n.name.split(".")[0] == "oracle"]
        elif isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "oracle":
            hits.append(node.module)
    return hits


def test_product_package_never_imports_the_oracle():
    for root in ("facodec_amd", "tools"):
        for dp, _, files in os.walk(os.path.join(REPO, root)):
            for f in files:
                if f.endswith(".py"):
                    assert _imports_oracle(os.path.join(dp, f)) == [], f"{dp}/{f} imports the oracle"


def _function_level_only(path, allowed):
    tree = ast.parse(open(path).read())
    for node in tree.body:                      # no module-level oracle import
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            mod = getattr(node, "module", None) or ",".join(n.name for n in node.names)
            assert not mod.startswith("oracle"), f"{path}: module-level oracle import"
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef):
            uses = any(isinstance(n, ast.ImportFrom) and n.module and n.module.startswith("oracle") for n in ast.walk(node))
            if uses:
                assert node.name in allowed, f"{path}: {node.name} imports the oracle"


def test_bench_and_entry_use_the_oracle_only_as_checker():
    _function_level_only(os.path.join(REPO, "bench.py"), {"cpu_baseline"})
    _function_level_only(os.path.join(REPO, "__graft_entry__.py"), {"smoke"})


# Environment variables and preprocessor conditions the package may read: deployment / resource configuration, and the second paths
# that tests drive through a child process's environment.  A tuning lever does not belong here: settle it, keep the
# winner as a constant and delete the switch.
FAC_NAMES_ALLOWED = {
    "FAC_LIB_PATH", "FAC_BUILD_TAG", "FAC_EXTRA_FLAGS",
    "FAC_NATIVE_RCCL", "FAC_FORCE_ALLREDUCE", "FAC_DIST_BACKEND", "FAC_BUCKET_MB", "FAC_EARLY_EXCHANGE",
    "FAC_QUANT_STREAMS", "FAC_DISC_STREAMS", "FAC_PRED_STREAMS", "FAC_MEL_STREAMS",
    "FAC_WGRAD_WS_GB", "FAC_LSTM_PERSIST_SPLIT_MAX_SCRATCH_GB",
    "FAC_WGRAD_NARROW", "FAC_WEIGHT_BATCH", "FAC_PW", "FAC_PW_SPLIT",
}


def test_fac_environment_reads_and_macro_conditions_are_the_allowed_ones():
    import glob
    import re
    pkg = os.path.join(REPO, "facodec_amd")
    files = glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True) + glob.glob(os.path.join(pkg, "csrc", "*"))
    found = set()
    for path in files:
        if os.path.isfile(path) and path.endswith((".py", ".hip", ".h")):
            for line in open(path):
                if re.search(r"os\.environ|getenv\s*\(|^\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    found |= set(re.findall(r"\bFAC_[A-Z0-9_]+", line))
    assert found == FAC_NAMES_ALLOWED, (sorted(found - FAC_NAMES_ALLOWED), sorted(FAC_NAMES_ALLOWED - found))
