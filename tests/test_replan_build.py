"""The replanning programs under tests/integration build against the installed
headers and libraries without a device (they run in test_gpu_replan_session.py)."""
import os

import pytest

from tests.test_abi import build_node_callsite


@pytest.mark.parametrize("src", ["node_replan.cpp", "replan_session_node.cpp"])
def test_replan_programs_compile(tmp_path, src):
    assert os.path.exists(build_node_callsite(tmp_path / src[:-4], src=src))
