"""csrc/bindings/ops.cpp turns a tensor into a pointer in its accessor section only.

Every binding takes its tensor arguments through the checked accessors between the BEGIN / END
TENSOR ACCESSORS markers (device, dtype, layout, size). This test reads the file as text and
holds it to that: outside the section, and outside the functions that carry raw IPC pointers as
int64 by design, no storage pointer is taken and no pointer cast is written.
"""
import re
from pathlib import Path

OPS_CPP = Path(__file__).resolve().parent.parent / "csrc" / "bindings" / "ops.cpp"
BEGIN = "// ==== BEGIN TENSOR ACCESSORS"
END = "// ==== END TENSOR ACCESSORS"

# raw device pointers of the IPC buffers travel as int64 (hipIpc handles, peer bases)
RAW_POINTER_FUNCTIONS = ("car_alloc", "car_free", "car_ipc_handle", "car_ipc_open", "car_ipc_close", "car_error",
                         "car_clear_error", "ep_ipc_view", "ep_ipc_stats", "ep_peers")
# the same for this one-line lambda of the schema block
RAW_POINTER_LINES = ('m.def("ep_ipc_error(int ptr) -> int"',)


def _without_function(text: str, name: str) -> str:
    """Drop the definition of the file-level function `name` (a one-liner, or up to the next
    closing brace in column 0)."""
    m = re.search(rf"^[\w:<>\*& ]+\b{name}\([^;{{]*\{{", text, flags=re.M)
    assert m, f"{name} not found"
    line_end = text.index("\n", m.end() - 1)
    if text[m.end() - 1:line_end].rstrip().endswith("}") and text[m.start():line_end].count("{") == \
            text[m.start():line_end].count("}"):
        end = line_end + 1
    else:
        end = text.index("\n}\n", m.end()) + 3
    return text[:m.start()] + text[end:]


def _split():
    text = OPS_CPP.read_text()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "accessor section markers"
    b, e = text.index(BEGIN), text.index(END)
    assert b < e
    return text, text[b:e], text[:b] + text[e:]


def _checked_rest() -> str:
    _, _, rest = _split()
    for name in RAW_POINTER_FUNCTIONS:
        rest = _without_function(rest, name)
    for line in RAW_POINTER_LINES:
        kept = [ln for ln in rest.splitlines() if line not in ln]
        assert len(kept) == len(rest.splitlines()) - 1, line
        rest = "\n".join(kept)
    return rest


def test_accessor_section_precedes_every_binding():
    text, section, _ = _split()
    first_impl = re.search(r'm\.impl\("(\w+)"', text).group(1)
    assert text.index(END) < text.index(f"void {first_impl}(")
    assert "data_ptr" in section and "struct Op" in section


def test_no_storage_pointer_outside_the_accessors():
    rest = _checked_rest()
    assert "data_ptr" not in rest
    assert "storage()" not in rest and "unsafeGetTensorImpl" not in rest


def test_no_pointer_helper_is_defined_outside_the_accessors():
    text, _, _ = _split()
    # the former free helpers bf(t) / u8(t): neither defined nor called anywhere
    assert not re.search(r"(?<![\w.:>])(bf|u8)\(", text)


def test_no_cast_of_tensor_storage_outside_the_accessors():
    # stronger than "no reinterpret_cast applied to a tensor": none at all is left
    rest = _checked_rest()
    assert "reinterpret_cast" not in rest
    assert not re.search(r"\(\s*(const\s+)?[\w:]+\s*\*\s*\)\s*\w+\.data_ptr", rest)


def test_removed_functions_held_the_raw_pointers():
    """The exemptions are really there (a renamed function must not silently leave the list)."""
    _, _, rest = _split()
    for name in ("car_alloc", "ep_ipc_view", "ep_peers", "ep_ipc_stats"):
        assert len(_without_function(rest, name)) < len(rest)
