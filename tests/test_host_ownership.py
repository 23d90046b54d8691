"""Every device allocation, page-locked allocation and event of a handle goes through its owner (csrc/agx_host_handle.hpp:
DeviceOwner), which is what frees them in agx_ocp_destroy: a bare allocation into a handle field would stay behind.  The host
files may call the runtime's allocators in the owner itself and in agx_host_alloc / agx_host_free (the caller's memory) only."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parents[1] / "agimus_controller_amd" / "csrc"
HOST_FILES = ("agimus_hip.hip", "agx_host_handle.hpp", "agx_host_traj.hpp")
CALL = re.compile(r"\b(hipMalloc\w*|hipHostMalloc|hipEventCreate\w*|hipFree\w*|hipHostFree|hipEventDestroy)\s*\(")


def _function_body(text, header):
    start = text.index(header)
    depth, i = 0, text.index("{", start)
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return start, j + 1
    raise AssertionError(header)


def raw_calls(texts):
    """[(file, line)] of runtime allocator calls outside DeviceOwner and agx_host_alloc / agx_host_free."""
    out = []
    for name, text in texts.items():
        allowed = []
        for header in ("class DeviceOwner {", "int agx_host_alloc(", "int agx_host_free("):
            if header in text:
                allowed.append(_function_body(text, header))
        for m in CALL.finditer(text):
            if not any(a <= m.start() < b for a, b in allowed):
                out.append((name, text.count("\n", 0, m.start()) + 1, m.group(1)))
    return out


def test_handle_resources_are_allocated_through_the_owner():
    texts = {n: (CSRC / n).read_text() for n in HOST_FILES}
    assert "class DeviceOwner {" in texts["agx_host_handle.hpp"] and "int agx_host_alloc(" in texts["agimus_hip.hip"]
    assert raw_calls(texts) == []


def test_the_scan_sees_a_bare_allocation():
    texts = {"x.hpp": "int f(agx_ocp *o) {\n  if (!o->d_hidx) HIPCHK(hipMalloc((void **)&o->d_hidx, sizeof(int) * (o->T + 1)));\n  return 0;\n}\n"}
    assert raw_calls(texts) == [("x.hpp", 2, "hipMalloc")]
