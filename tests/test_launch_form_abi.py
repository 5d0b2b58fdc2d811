"""CPU checks of lp_last_launch_form (include/lp_hip.h): argument validation returns the error code without a GPU, the record is zeroed before any
launch, the call is thread-local host state, and the ABI version is unchanged.  No GPU calls."""
import ctypes
import threading


def test_argument_validation_without_a_gpu():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    assert l.lp_abi_version() == 12
    rec = (ctypes.c_int * 20)()
    assert l.lp_last_launch_form(None, 20) == -1 and b'null' in l.lp_last_error()
    assert l.lp_last_launch_form(ctypes.addressof(rec), 19) == -1 and b'capacity' in l.lp_last_error()
    assert l.lp_last_launch_form(ctypes.addressof(rec), 0) == -1
    assert l.lp_last_launch_form(ctypes.addressof(rec), -5) == -1
    assert l.lp_last_launch_form(ctypes.addressof(rec), 20) == 0


def test_record_is_zero_before_any_launch_and_nothing_beyond_it_is_written():
    from latent_pose_reenactment_amd import _lib, hipops
    l = _lib.lib()
    out = {}

    def fresh_thread():            # a thread that never launched: its record is the initial one, whatever the main thread has done
        rec = (ctypes.c_int * 24)(*([-7] * 24))
        out['rc'] = l.lp_last_launch_form(ctypes.addressof(rec), 24)
        out['rec'] = list(rec)
        out['dict'] = hipops.last_launch_form()
        # a rejected conv call (argument validation, before any device work) leaves the record alone
        out['rc_conv'] = l.lp_conv16_fwd(None, None, None, None, None, None, None, None, None, 1, 4, 4, 64, 64, 64, 128, 3, 0, 0, 0, None, None, None, 0,
                                         None, 0, None, None)
        rec = (ctypes.c_int * 20)(*([-7] * 20))
        out['rc2'] = l.lp_last_launch_form(ctypes.addressof(rec), 20)
        out['rec2'] = list(rec)
    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert out['rc'] == 0 and out['rec'] == [0] * 20 + [-7] * 4
    assert out['dict'] == {'what': None}
    assert out['rc_conv'] == -1 and out['rc2'] == 0 and out['rec2'] == [0] * 20
