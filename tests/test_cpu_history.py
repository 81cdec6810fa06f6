"""The enumerators of a context's persistent memory (context.h: for_each_workspace and its siblings) list every DevBuf of
their struct, and nothing releases a DevBuf except through them: what stk_destroy frees and what the debug_poison option
fills (tests/test_gpu_history.py) is one list per struct. Parsed from the sources, like test_cpu_local_norm.py parses the
header's structs."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libstacker_rs_amd", "csrc")


def _src(name):
    text = open(os.path.join(CSRC, name)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _struct_body(text, name):
    m = re.search(r"struct\s+%s\s*\{" % name, text)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def _devbuf_members(body):
    """Names declared as `DevBuf a, b;` or `std::vector<DevBuf> a;` at the top level of a struct body."""
    flat, depth = "", 0
    for ch in body:                                            # drop nested structs' bodies
        depth += ch == "{"
        if depth == 0:
            flat += ch
        depth -= ch == "}"
    names = []
    for stmt in flat.split(";"):
        m = re.fullmatch(r"(?:std::vector<DevBuf>|DevBuf)\s+([^()]+)", stmt.strip(), re.S)
        if m:
            names += [n.strip() for n in m.group(1).split(",")]
    assert all(re.fullmatch(r"\w+", n) for n in names), names
    return names


def _function_body(text, signature):
    m = re.search(signature + r"[^;{]*\{", text)
    assert m, signature
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


STRUCTS = [   # (file of the struct, struct, file of the enumerator, the enumerator's signature, how a member is named in it, its count)
    ("context.h", "stk_ctx", "context.h", r"inline void for_each_workspace\(stk_ctx\* ctx,", "&ctx->%s", 22),
    ("keypoint.cpp", "KeypointWorkspace", "keypoint.cpp", r"void for_each_workspace\(KeypointWorkspace\* k,", "&k->%s", 16),
    ("homography.cpp", "HgWorkspace", "homography.cpp", r"void for_each_workspace\(HgWorkspace\* w,", "&w->%s", 8),
    ("multi.cpp", "MultiState", "multi.cpp", r"void stk::for_each_workspace\(MultiState\* ms,", "&ms->%s", 3),
]


def test_every_devbuf_member_is_enumerated():
    for sfile, struct, efile, signature, ref, count in STRUCTS:
        members = _devbuf_members(_struct_body(_src(sfile), struct))
        assert len(members) == count and len(set(members)) == count, (struct, members)
        body = _function_body(_src(efile), signature)
        listed = re.findall(re.escape(ref).replace("%s", r"(\w+)") + r"\b", body)
        assert sorted(listed) == sorted(members), (struct, sorted(set(members) ^ set(listed)))


def test_every_pinned_host_block_is_enumerated():
    ctx = _function_body(_src("context.h"), r"inline void for_each_workspace\(stk_ctx\* ctx,")
    assert "host(ctx->host_done," in ctx and "host(ctx->files_block," in ctx
    kp_struct = _struct_body(_src("keypoint.cpp"), "KeypointWorkspace")
    blocks = re.findall(r"\*\s*(host_\w+)\s*=\s*nullptr", kp_struct)
    assert sorted(blocks) == ["host_final", "host_kept", "host_kept_cnt", "host_knn", "host_sel", "host_states"]
    kp = _function_body(_src("keypoint.cpp"), r"void for_each_workspace\(KeypointWorkspace\* k,")
    for b in blocks:
        assert "host(k->%s," % b in kp, b
    assert "host(w->pinned," in _function_body(_src("homography.cpp"), r"void for_each_workspace\(HgWorkspace\* w,")


def test_nothing_releases_a_devbuf_outside_the_enumerators():
    """The one release() call of a workspace is workspace_release_dev, which only the destroys hand to an enumerator; the
    RCCL self-test's local buffers (bufs[r], no member of any struct) are the other caller of DevBuf::release."""
    for name in ("context.h", "stacker.cpp", "keypoint.cpp", "homography.cpp", "multi.cpp"):
        text = _src(name)
        assert "->release()" not in text, name
        calls = re.findall(r"[\w\[\]\)]+\s*\.\s*release\(\)", text)
        allowed = {"context.h": ["b.release()"], "multi.cpp": ["bufs[r].release()"]}.get(name, [])
        assert calls == allowed, (name, calls)
    for name, fn, signature in (("stacker.cpp", "stk_destroy", r"void stk_destroy\(stk_ctx\* ctx\)"),
                                ("keypoint.cpp", "keypoint_workspace_destroy", r"void keypoint_workspace_destroy\(KeypointWorkspace\* k\)"),
                                ("homography.cpp", "hg_workspace_destroy", r"void hg_workspace_destroy\(HgWorkspace\* w\)"),
                                ("multi.cpp", "multi_destroy", r"void multi_destroy\(stk_ctx\* ctx\)")):
        body = _function_body(_src(name), signature)
        assert re.search(r"for_each_workspace\(\w+, workspace_release_dev", body), fn
        assert "hipFree" not in body and "hipHostFree" not in body, fn
    # the workspaces are DevBufs everywhere: no other file frees device memory behind their back
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".cpp", ".h", ".hip")) and name != "context.h":
            assert not re.search(r"\bhipFree\(", _src(name)), name


def test_the_header_and_the_integration_notes_name_the_debug_hook():
    hdr = open(os.path.join(ROOT, "include", "stacker.h")).read()
    options = hdr[hdr.index("Tuning knobs."):hdr.index("stk_status  stk_set_option(")]
    counters = hdr[hdr.index("Device-side event counters"):hdr.index("stk_status  stk_get_counter(")]
    assert '"debug_poison"' in options
    assert '"workspaces_empty"' in counters and '"debug_poison_bytes"' in counters
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("debug_poison", "workspaces_empty", "debug_poison_bytes"):
        assert name in notes, name
    # and the engine knows the names it documents
    src = _src("stacker.cpp")
    for name in ("debug_poison", "workspaces_empty", "debug_poison_bytes"):
        assert '"%s"' % name in src, name
