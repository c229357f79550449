"""Class / method rows streamed to the SQLite writer while the Java scan is
still parsing (``DMCP_STREAM_ROWS``, native/srcscan) must leave exactly what
the after-scan emission leaves: the same rows in the same id order, the same
graph, last-file-wins for colliding identifiers, and a rolled-back swap when
the analysis fails after rows were queued."""
import json
import os
import shutil
import sqlite3

import pytest

from conftest import make_app
from dmcp.enrich.backend import NullBackend
from dmcp.index.source import MemoryTree
from dmcp.models.domain import ProjectStatus
from dmcp.parsers.base import ParsedProject
from dmcp.utils import synth
from dmcp.utils.errors import DomainError

JAVA_ROOT = os.path.join("src", "main", "java")


def _java_files(root):
    out = []
    for d, _, names in os.walk(os.path.join(root, JAVA_ROOT)):
        out += [os.path.join(d, n) for n in names if n.endswith(".java")]
    return sorted(out)


def _java_repo(root, n):
    """A generated Spring repo cut down to exactly ``n`` Java files (the
    generator writes whole domains of 8 classes)."""
    synth.java_spring_repo(root, max(n, 1), commit=False)
    files = _java_files(root)
    assert len(files) >= n
    for p in files[n:]:
        os.remove(p)
    synth._git_commit(root)
    return root


def _app(tmp, threads):
    return make_app(tmp, backend=NullBackend(), enrich_backend="null", require_enrichment_for_analyze=False,
                    parser_threads=threads)


def _strip_class_ids(x):
    if isinstance(x, dict):
        return {k: _strip_class_ids(v) for k, v in x.items() if k != "classId"}
    if isinstance(x, list):
        return [_strip_class_ids(v) for v in x]
    return x


def _snapshot(db_path):
    """The three row tables ordered by id, ids replaced by their rank (class
    and method ids share one ranking: one generator hands out a class id, then
    its methods' ids), timestamps and the project id left out; plus the graph
    JSON without class ids."""
    con = sqlite3.connect(db_path)
    try:
        classes = con.execute("SELECT id, full_class_name, simple_name, package_name, class_type, description, "
                              "source_file, commit_hash FROM source_classes ORDER BY id").fetchall()
        methods = con.execute("SELECT id, class_id, method_name, description, business_logic, exceptions, "
                              "http_method, http_path, line_number FROM source_methods ORDER BY id").fetchall()
        params = con.execute("SELECT id, method_id, position, class_id FROM method_parameters ORDER BY id").fetchall()
        graphs = [r[0] for r in con.execute("SELECT g.graph_data FROM project_graphs g JOIN projects p "
                                            "ON p.id = g.project_id ORDER BY p.name")]
    finally:
        con.close()
    rank = {i: k for k, i in enumerate(sorted([c[0] for c in classes] + [m[0] for m in methods]))}
    prank = {p[0]: k for k, p in enumerate(params)}
    return {
        "classes": [(rank[c[0]],) + c[1:] for c in classes],
        "methods": [(rank[m[0]], rank[m[1]]) + m[2:] for m in methods],
        "params": [(prank[p[0]], rank[p[1]], p[2], rank[p[3]]) for p in params],
        "class_order": [c[1] for c in classes],
        "graphs": [_strip_class_ids(json.loads(g)) for g in graphs],
    }


def _analyze(tmp, repo, threads, stream, monkeypatch):
    """One analysis into a fresh database; (snapshot, files the scan streamed)."""
    monkeypatch.setenv("DMCP_STREAM_ROWS", "1" if stream else "0")
    seen = {}
    real = MemoryTree.scan_objects

    def spy(self, *a, **kw):
        doc = real(self, *a, **kw)
        seen["streamed"] = doc["stats"].get("streamedFiles")
        seen["rows"] = doc["stats"]["phaseUs"].get("rows")
        seen["has_ids"] = "rowIds" in doc
        return doc

    monkeypatch.setattr(MemoryTree, "scan_objects", spy)
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)
    os.makedirs(tmp)
    from pathlib import Path
    app = _app(Path(tmp), threads)
    try:
        r = app.indexer.analyze_project(str(repo))
        assert r.success, r.message
    finally:
        app.close()
    assert seen["has_ids"] and seen["rows"] is not None  # the native scan wrote the rows in both modes
    return _snapshot(os.path.join(tmp, "db.sqlite")), seen["streamed"]


def _assert_equivalent(tmp_path, repo, threads, monkeypatch, n_files=None):
    on, streamed = _analyze(str(tmp_path / "on"), repo, threads, True, monkeypatch)
    off, not_streamed = _analyze(str(tmp_path / "off"), repo, threads, False, monkeypatch)
    assert not_streamed == 0
    if n_files is not None:
        assert streamed == n_files  # every Java file's rows left through the scan's sink
    assert on["class_order"] == off["class_order"]  # ids ascend in the same class order
    assert on["classes"] == off["classes"]
    assert on["methods"] == off["methods"]
    assert on["params"] == off["params"]
    assert on["graphs"] == off["graphs"]
    return on


@pytest.fixture(scope="module")
def java_repos(tmp_path_factory):
    made = {}

    def get(n):
        if n not in made:
            made[n] = _java_repo(str(tmp_path_factory.mktemp(f"java{n}") / "shop"), n)
        return made[n]

    return get


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 600])
def test_java_rows_equal_streamed_and_after_scan(tmp_path, java_repos, monkeypatch, n, threads):
    snap = _assert_equivalent(tmp_path, java_repos(n), threads, monkeypatch, n_files=n)
    assert len(snap["classes"]) == n
    if n:
        assert snap["methods"] and snap["graphs"][0]["nodes"]


def test_colliding_identifiers_last_file_wins(tmp_path, monkeypatch):
    repo = str(tmp_path / "shop")
    synth.java_spring_repo(repo, 8, commit=False)
    base = os.path.join(repo, JAVA_ROOT)
    # both paths give the identifier a.b.C; the walk lists a/ before a.b/
    synth._write(os.path.join(base, "a", "b", "C.java"),
                 "package a.b;\n\n@org.springframework.stereotype.Service\npublic class C {\n"
                 "    public void first() {}\n    public void alsoFirst() {}\n}\n")
    synth._write(os.path.join(base, "a.b", "C.java"),
                 "package a.b;\n\n@org.springframework.stereotype.Repository\npublic class C {\n"
                 "    public void second() {}\n}\n")
    synth._git_commit(repo)
    snap = _assert_equivalent(tmp_path, repo, 8, monkeypatch, n_files=len(_java_files(repo)))
    rows = [c for c in snap["classes"] if c[1] == "a.b.C"]
    assert len(rows) == 1 and rows[0][6] == "src/main/java/a.b/C.java"
    cid = rows[0][0]
    assert [m[2] for m in snap["methods"] if m[1] == cid] == ["second"]


def test_unparsable_files_among_good_ones(tmp_path, monkeypatch):
    repo = str(tmp_path / "shop")
    synth.java_spring_repo(repo, 24, commit=False)
    base = os.path.join(repo, JAVA_ROOT, "co", "acme", "shop")
    synth._write(os.path.join(base, "Empty.java"), "")
    synth._write(os.path.join(base, "Unbalanced.java"), "package co.acme.shop;\npublic class Unbalanced { void f( {{{ \"")
    with open(os.path.join(base, "Binary.java"), "wb") as f:
        f.write(bytes(range(256)) * 8 + b"\xff\xfe class \x00")
    synth._git_commit(repo)
    snap = _assert_equivalent(tmp_path, repo, 8, monkeypatch, n_files=len(_java_files(repo)))
    assert {"co.acme.shop.Empty", "co.acme.shop.Unbalanced", "co.acme.shop.Binary"} <= set(snap["class_order"])


def test_failure_after_rows_streamed_rolls_back(tmp_path, java_repos, monkeypatch):
    monkeypatch.setenv("DMCP_STREAM_ROWS", "1")
    repo = java_repos(600)
    app = _app(tmp_path, 8)
    db = str(tmp_path / "db.sqlite")
    try:
        r = app.indexer.analyze_project(str(repo))
        assert r.success
        before = _snapshot(db)
        con = sqlite3.connect(db)
        ids_before = [x[0] for x in con.execute("SELECT id FROM source_classes ORDER BY id")]
        con.close()

        def boom(self):
            raise RuntimeError("graph build failed")

        monkeypatch.setattr(ParsedProject, "build_graph", boom)
        with pytest.raises(DomainError):
            app.indexer.analyze_project(str(repo))  # its 600 files' rows were queued before the failure
        monkeypatch.undo()
        # the writer's transaction is over (its thread has rolled back and
        # was joined): the write lock is free at once
        con = sqlite3.connect(db, timeout=0)
        try:
            con.execute("BEGIN IMMEDIATE")
            con.execute("ROLLBACK")
            ids_after = [x[0] for x in con.execute("SELECT id FROM source_classes ORDER BY id")]
        finally:
            con.close()
        assert ids_after == ids_before  # the very rows of the first analysis, not equal new ones
        after = _snapshot(db)
        assert after["classes"] == before["classes"] and after["methods"] == before["methods"]
        assert after["params"] == before["params"]
        assert app.repos.projects.find_by_id(r.project_id).status is ProjectStatus.ERROR
    finally:
        app.close()


def test_typescript_rows_equal_in_both_modes(tmp_path, monkeypatch):
    repo = str(tmp_path / "nest")
    synth.nestjs_repo(repo, n_modules=5)
    on, streamed = _analyze(str(tmp_path / "on"), repo, 8, True, monkeypatch)
    off, _ = _analyze(str(tmp_path / "off"), repo, 8, False, monkeypatch)
    assert streamed == 0  # TypeScript compacts its file list after the parse: rows follow the scan
    assert on["classes"] and on["methods"]
    for k in ("class_order", "classes", "methods", "params", "graphs"):
        assert on[k] == off[k]
