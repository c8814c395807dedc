"""The three loss entries (tg_net_loss_grad, tg_net_loss_grad_sliced, tg_net_loss_grad_s25) apply the same argument
rules, in the same order, with the same words: each refusal below gives the same code from all three, and the same
tg_last_error() once the entry's own name (and, for the workspace's size, its two byte counts) is taken out.  Each entry
gets a configuration its family accepts, so every refusal comes from the call's arguments.  No GPU needed."""
import ctypes as C
import re

from mat_mul_amd import _lib, net, ops

from net_ref import CONFIGS as CONFIGS_S4
from net_ref import dims
from net_s16_ref import CONFIGS as CONFIGS_S16
from net_s25_train_family import ROWS as ROWS_S25

B = 4
POINTERS = ("theta", "pos_fix", "frames", "scalars", "g_action", "g_value", "ws", "losses", "status")


def _entries():
    lib = _lib.lib
    return (
        ("tg_net_loss_grad", lib.tg_net_loss_grad, net.check_config(dims(CONFIGS_S4["a"])),
         ops.net_train_workspace_size),
        ("tg_net_loss_grad_sliced", lib.tg_net_loss_grad_sliced, net.check_config(dims(CONFIGS_S16["a16"])),
         ops.net_train_sliced_workspace_size),
        ("tg_net_loss_grad_s25", lib.tg_net_loss_grad_s25, net.check_config(dims(ROWS_S25["a25"]), ops.net_s25_check),
         ops.net_train_s25_workspace_size),
    )


def _refusals(name, fn, cfg, need):
    """(code, text without the entry's name) of every refusal, in the order of the rules."""
    p, ws = C.c_void_p(64), C.c_void_p(256)  # never dereferenced: every call below is refused before any launch

    def call(theta=p, pos_fix=p, frames=p, i8=1, scalars=p, g_action=p, g_value=p, B=B, wp=1.0, wv=1000.0, dp=0.5, ws=ws,
             ws_bytes=need, grad=p, losses=p, status=p):
        rc = fn(C.byref(cfg), theta, pos_fix, frames, i8, scalars, g_action, g_value, B, wp, wv, dp, 0, 0, None, None, ws,
                ws_bytes, grad, losses, status, None)
        text = _lib.lib.tg_last_error().decode()
        assert text.startswith(name + ": "), text
        return rc, text[len(name) + 2:]

    out = {"B": call(B=0), "dropout": call(dp=1.0), "weight": call(wp=float("nan")), "i8": call(i8=2)}
    for ptr in POINTERS:
        out["null " + ptr] = call(**{ptr: None})
    out["workspace 128"] = call(ws=C.c_void_p(384))  # aligned to 128 bytes, not to 256
    out["theta 2"] = call(theta=C.c_void_p(66))
    rc, text = call(ws_bytes=need - 1)
    assert [int(x) for x in re.findall(r"\d+", text)] == [need - 1, need], text
    out["workspace size"] = (rc, re.sub(r"\d+", "N", text))
    out["B and null theta"] = call(B=0, theta=None)  # two faults at once: the earlier rule's words
    return out


def test_the_three_loss_entries_refuse_alike():
    got = {name: _refusals(name, fn, cfg, size(cfg, B)) for name, fn, cfg, size in _entries()}
    whole = got["tg_net_loss_grad"]
    assert all(rc == -1 for rc, _ in whole.values()), whole
    assert len({text for _, text in whole.values()}) == 7, whole  # one text per rule: the nulls share one, the alignments one
    for name, cases in got.items():
        for case, want in whole.items():
            assert cases[case] == want, (name, case)
    assert whole["B and null theta"] == whole["B"] and "B=0" in whole["B"][1]
    assert "dropout_p=1" in whole["dropout"][1] and "not finite" in whole["weight"][1] and "frames_is_i8=2" in whole["i8"][1]
    assert "null" in whole["null theta"][1] and "aligned" in whole["theta 2"][1]
    assert whole["theta 2"] == whole["workspace 128"]
    assert whole["workspace size"][1] == "workspace of N bytes, N needed"
