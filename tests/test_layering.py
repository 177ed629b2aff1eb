"""The package's layering: the server, the ops, the models, the runtime and
the utilities stand below the benchmark workloads and never import them."""

import ast
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWER = ('server', 'ops', 'models', 'runtime', 'utils')


def _imports(path, package):
    """Absolute names of every module ``path`` (a module of ``package``)
    imports, relative imports resolved."""
    with open(path, encoding='utf-8') as fh:
        tree = ast.parse(fh.read(), path)
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom):
            base = package.split('.')
            if node.level:
                base = base[:len(base) - (node.level - 1)]
                mod = '.'.join(base + ([node.module] if node.module else []))
            else:
                mod = node.module
            yield mod
            for a in node.names:
                yield mod + '.' + a.name


def _modules():
    for layer in LOWER:
        top = os.path.join(ROOT, 'zkmi', layer)
        for d, _, fs in os.walk(top):
            for f in fs:
                if f.endswith('.py'):
                    path = os.path.join(d, f)
                    rel = os.path.relpath(d, ROOT).replace(os.sep, '.')
                    yield path, rel


def test_lower_layers_do_not_import_the_benchmark():
    found = [(os.path.relpath(path, ROOT), name)
             for path, package in _modules()
             for name in _imports(path, package)
             if name == 'zkmi.bench' or name.startswith('zkmi.bench.')]
    assert found == []
    assert len(list(_modules())) > 10        # the walk found the package


def test_front_end_import_leaves_the_benchmark_unloaded():
    code = ('import sys, zkmi.server.gpu; '
            'print("zkmi.bench.synthetic" in sys.modules)')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-1] == 'False', r.stdout


def test_benchmark_module_still_exports_what_the_driver_uses():
    from zkmi.bench import synthetic as S
    assert hasattr(S, 'GpuTree') and hasattr(S, 'GetPipeline')
