"""CPU-only side of instance masks (rt_scene_set_instance_mask(s), rt_scene_get_instance_masks): the exports, their binding and their
citations, and the argument checks that need no device.  (The GPU side: tests/test_gpu_instance_masks.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_scene_set_instance_mask", "rt_scene_set_instance_masks", "rt_scene_get_instance_masks")


def test_exports_and_their_argument_types(capi):
    u32, p = C.c_uint32, C.c_void_p
    want = {"rt_scene_set_instance_mask": [p, u32, C.c_uint8], "rt_scene_set_instance_masks": [p, u32, u32, p],
            "rt_scene_get_instance_masks": [p, u32, u32, p]}
    lib = capi.lib()
    for name in NEW:
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and args == want[name], name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(NEW) <= exported, set(NEW) - exported
    for method in ("set_mask", "set_masks", "masks"):
        assert callable(getattr(capi.Scene, method))


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared under a comment that says EXTENSION and cites the instance descriptor (TopLevelASGenerator.cpp:344-362); the
    block names the TraceRay call sites whose inclusion mask makes "non-zero" mean "visible"; the C++ mirror has the two methods"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in NEW:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        comments = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)
        near = " ".join(comments[-2:])
        assert "EXTENSION" in near and "TopLevelASGenerator.cpp:344-362" in near, name
    block = text[text.index("Instance masks"):text.index("int rt_scene_get_instance_masks")]
    for cite in ("ProgressiveRaytracing.hlsl:34,53", "RaytracingCommon.hlsli:94", "RealtimeRaytracing.hlsl:42,61", "0xFF", "RT_ERR_STATE", "no instance is visible"):
        assert cite in block, cite
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    assert re.search(r"void setInstanceMask\(uint32_t \w+, uint8_t \w+\)", mirror) and re.search(r"uint8_t getInstanceMask\(uint32_t \w+\) const", mirror)
    assert "EXTENSIONS" in mirror[:mirror.index("void setInstanceMask")]
    assert mirror.index("void setTransform") < mirror.index("void setInstanceMask") < mirror.index("void update(")


def test_calls_refuse_null_arguments(capi):
    """argument checks need no device"""
    m = np.zeros(4, np.uint8)
    lib = capi.lib()
    invalid = -1                                       # RT_ERR_INVALID_ARG (include/dxr_amd_types.h)
    assert lib.rt_scene_set_instance_mask(None, 0, 0xFF) == invalid
    assert lib.rt_scene_set_instance_masks(None, 0, 1, m.ctypes.data_as(C.c_void_p)) == invalid
    assert lib.rt_scene_set_instance_masks(None, 0, 0, None) == invalid
    assert lib.rt_scene_get_instance_masks(None, 0, 1, m.ctypes.data_as(C.c_void_p)) == invalid
