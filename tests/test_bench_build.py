"""bench.py calls __graft_entry__.build() only where it may write build()'s lock file: in a tree built by another user the
lock is not writable, and bench.py runs the build that is there instead of failing before the first step.  CPU only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_fresh_tree_may_build(tmp_path):
    assert bench.may_build(str(tmp_path / "build" / "obj"))        # nothing there yet: the writable tree root decides
    (tmp_path / "build" / "obj").mkdir(parents=True)
    (tmp_path / "build" / "obj" / ".lock").write_text("")
    assert bench.may_build(str(tmp_path / "build" / "obj"))


@pytest.mark.skipif(os.geteuid() == 0, reason="root writes any file whatever its mode")
def test_tree_built_by_another_user_is_not_built_in(tmp_path):
    obj = tmp_path / "build" / "obj"
    obj.mkdir(parents=True)
    (obj / ".lock").write_text("")
    (obj / ".lock").chmod(0o444)
    try:
        assert not bench.may_build(str(obj))
        (obj / ".lock").unlink()
        obj.chmod(0o555)
        assert not bench.may_build(str(obj))
    finally:
        obj.chmod(0o755)
