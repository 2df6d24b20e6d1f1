"""The layout of the Python package (module map): which module may import which, where
an import may sit inside a function, where torch may be named, that `import blueberry_amd` stays
light, that every name of `blueberry_amd` and `blueberry_amd.solver` is still there and is the
object of its home module, and that the two rank rules exist once.  Read from the sources with
`ast`: no library, no GPU."""
import ast
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blueberry_amd")

# module -> the package modules it may import at module level (the table of DESIGN.md).  `triples`
# also reads `plan` (the layout and the type codes, for `DeviceTriples.tiles`) and `engine` (the KR
# vectors' check, for the graph calls); the type codes live in `plan` because `layout_info` reads them.
LEAVES = {"_lib", "utils"}
MAY_IMPORT = {
    "_lib": LEAVES, "utils": LEAVES, "compare": LEAVES, "resolution": LEAVES, "stats": LEAVES,
    "ranks": set(),
    "band": LEAVES | {"ranks"},
    "datatypes": LEAVES | {"ranks", "resolution"},
    "plan": {"_lib"},
    "engine": {"_lib", "ranks", "plan"},
    "triples": {"_lib", "ranks", "datatypes", "plan", "engine"},
    "landmark": {"_lib", "ranks", "triples"},
    "exchange": {"ranks"},
    "fithic": {"_lib", "ranks", "datatypes", "triples"},
}
MAY_IMPORT["solver"] = set(MAY_IMPORT)
MAY_IMPORT["__init__"] = set(MAY_IMPORT) | {"solver"}

LATE = {("datatypes", "fithic"), ("triples", "fithic")}     # the estimator takes the type that calls it
TORCH = {"ranks", "exchange", "engine", "band"}             # and only inside functions

SOLVER_NAMES = {
    "triples": ["DeviceTriples", "GeodesicRows", "TriplesBalance", "balance_triples", "coarsen_triples"],
    "landmark": ["LandmarkInfo", "landmark_choice", "landmark_coefficients", "landmark_start"],
    "engine": ["GroupEngine", "HipEngine", "RankDeficient"],
    "plan": ["ALPHA_MAX", "ALPHA_MIN", "block_degrees", "block_step_factors", "degree_step_factors",
             "layout_info", "loglog_slope", "loglog_totals", "max_degree", "next_alpha",
             "tiles_from_blocks", "tiles_from_entries", "weighted_steps"],
    "exchange": ["allreduce_exchange", "allreduce_exchange_host", "comm_reuse", "run_iterations",
                 "select_exchange"],
    "datatypes": ["check_balance_args", "check_coarsen_args", "triples_buffer"],
    "solver": ["FitScore", "StructureSolver", "spectral_init"],
}
SOLVER_MODULES = ["contextlib", "math", "numpy", "os", "sys"]       # public names too, as they were
PACKAGE_NAMES = {
    "utils": ["HIGH_FITHIC_CUTOFF", "LOW_FITHIC_CUTOFF", "Q_LOWER_BOUND", "Q_UPPER_BOUND"],
    "band": ["count_band_regions"],
    "datatypes": ["ContactMap", "EigenNoConvergence", "FithicContactMap", "shortest_paths"],
    "compare": ["StructureComparison", "compare_structures"],
    "fithic": ["FitHiC", "binomial_sf"],
    "resolution": ["coarsen_structure", "prolong_structure"],
    "engine": ["HipEngine", "RankDeficient"],
    "landmark": ["landmark_coefficients", "landmark_start"],
    "solver": ["FitScore", "StructureSolver"],
    "stats": ["benjamini_hochberg", "downsample", "q_values"],
    "triples": ["DeviceTriples", "GeodesicRows", "TriplesBalance", "balance_triples", "coarsen_triples"],
}


def _sources():
    return {f[:-3]: open(os.path.join(PKG, f)).read() for f in sorted(os.listdir(PKG)) if f.endswith(".py")}


def _imports(tree):
    """(node, inside a function?) of every import statement."""
    def walk(node, inside):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.Import, ast.ImportFrom)):
                yield child, inside
            yield from walk(child, inside or isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef,
                                                                 ast.Lambda)))
    return walk(tree, False)


def _package_targets(node):
    """The package modules an import statement names."""
    if isinstance(node, ast.ImportFrom):
        if node.level == 1:
            return [node.module] if node.module else [a.name for a in node.names]
        if node.level == 0 and node.module and node.module.split(".")[0] == "blueberry_amd":
            rest = node.module.split(".")[1:]
            return rest[:1] if rest else [a.name for a in node.names]
        assert node.level == 0, "an import from above the package"
        return []
    return [a.name.split(".")[1] for a in node.names if a.name.startswith("blueberry_amd.")]


def _edges(late):
    out = set()
    for mod, text in _sources().items():
        for node, inside in _imports(ast.parse(text)):
            if inside == late:
                out |= {(mod, t) for t in _package_targets(node)}
    return out


def test_module_level_imports_follow_the_table_and_form_no_cycle():
    assert set(_sources()) == set(MAY_IMPORT), "a module the table does not know, or one gone"
    edges = _edges(late=False)
    bad = sorted((a, b) for a, b in edges if b not in MAY_IMPORT[a])
    assert not bad, "imports the table does not allow: %r" % bad
    graph = {m: {b for a, b in edges if a == m} for m in MAY_IMPORT}
    done, path = set(), []

    def visit(m):
        assert m not in path, "import cycle: %s" % " -> ".join(path[path.index(m):] + [m])
        if m not in done:
            path.append(m)
            for b in sorted(graph[m]):
                visit(b)
            path.pop()
            done.add(m)
    for m in sorted(graph):
        visit(m)


def test_late_package_imports_are_the_two_real_cycles():
    assert _edges(late=True) == LATE


def test_torch_is_named_only_inside_functions_of_four_modules():
    found = set()
    for mod, text in _sources().items():
        for node, inside in _imports(ast.parse(text)):
            names = [node.module or ""] if isinstance(node, ast.ImportFrom) else [a.name for a in node.names]
            if any(n.split(".")[0] == "torch" for n in names):
                assert inside, "%s imports torch at module level (line %d)" % (mod, node.lineno)
                found.add(mod)
    assert found == TORCH


def test_import_of_the_package_stays_light():
    code = ("import sys; sys.path.insert(0, %r); import blueberry_amd\n"
            "heavy = [m for m in ('torch', 'torch.distributed', 'scipy', 'matplotlib', 'pandas')\n"
            "         if m in sys.modules]\n"
            "assert not heavy, heavy\nprint('ok')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _check_names(holder, names_by_home):
    for home, names in names_by_home.items():
        module = importlib.import_module("blueberry_amd." + home)
        for name in names:
            obj = getattr(holder, name)
            assert obj is getattr(module, name), (holder.__name__, name)
            assert getattr(obj, "__module__", module.__name__) == module.__name__, (name, obj.__module__)


def test_every_name_is_still_there_and_is_its_home_modules_object():
    import blueberry_amd
    from blueberry_amd import ranks, solver
    assert sum(len(v) for v in SOLVER_NAMES.values()) + len(SOLVER_MODULES) == 41
    _check_names(solver, SOLVER_NAMES)
    for name in SOLVER_MODULES:
        assert getattr(solver, name) is importlib.import_module(name)
    assert solver._sum_over_ranks is ranks.sum_over_ranks
    assert sum(len(v) for v in PACKAGE_NAMES.values()) == 29
    _check_names(blueberry_amd, PACKAGE_NAMES)


def test_the_rank_rules_are_written_once():
    for needle in ('"LOCAL_RANK"', 'sys.modules.get("torch.distributed")'):
        assert [m for m, text in _sources().items() if needle in text] == ["ranks"], needle
