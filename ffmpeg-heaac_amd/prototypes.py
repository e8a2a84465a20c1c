"""The C prototypes of libheaac_amd.so as ctypes sees them: lib() applies them once, right after it loads the library, so
every call through the binding, the tests and the tools is marshalled alike -- a bare Python int goes over as the size_t,
float or double the header declares, and a pointer result comes back whole.  Nothing else may assign argtypes / restype on
this library's functions; tests/test_binding_prototypes.py compares the table with include/*.h."""
import ctypes as C

# every pointer (handles, records, out-parameters, void *stream) is P; S is a `const char *` result
P, S, I, Z, F, D = C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_float, C.c_double

# name: (restype, argtypes), in the order of the headers
PROTOTYPES = {
    # heaac_dsp.h
    "heaac_device_create": (I, [P, Z]),
    "heaac_device_destroy": (None, [P]),
    "heaac_device_workspace_bytes": (Z, [Z]),
    "heaac_strerror": (S, [I]),
    "heaac_imdct_half_batch": (I, [P, I, P, P, Z, P]),
    "heaac_lc_decode_batch": (I, [P, I, P, P, P, P, P, I, Z, P]),
    "heaac_lc_decode_streams": (I, [P, I, P, P, P, P, P, I, Z, Z, P]),
    "heaac_lc_decode_streams_ex": (I, [P, I, P, P, P, P, P, I, Z, Z, P, P]),
    "heaac_pcm_interleave_batch": (I, [P, I, P, I, I, P, Z, P]),
    "heaac_couple_after_imdct_batch": (I, [P, I, P, P, P, P, Z, P]),
    "heaac_he_decode_batch": (I, [P, I, P, P, P, P, Z, P, P, P, P, I, Z, P]),
    "heaac_he_decode_batch_ex": (I, [P, I, I, P, P, P, P, Z, P, P, P, P, I, Z, P]),
    "heaac_he_decode_streams": (I, [P, I, I, P, P, P, P, Z, P, P, P, P, I, Z, Z, P]),
    "heaac_he_decode_streams_ex": (I, [P, I, I, P, P, P, P, Z, P, P, P, P, I, Z, Z, P, P]),
    "heaac_validate_frame": (I, [I, P, P, Z, P]),
    "heaac_he_check_batch": (I, [P, I, P, P, Z, P, Z, P, P, P]),
    "heaac_qmf_analysis_batch": (I, [P, P, P, P, P, F, Z, P]),
    "heaac_qmf_synthesis_batch": (I, [P, P, P, P, P, F, F, Z, P]),
    "heaac_qmf_synthesis_ds_batch": (I, [P, P, P, P, P, F, F, Z, P]),
    "heaac_spectral_tools_batch": (I, [P, I, P, P, P, P, P, P, Z, P]),
    "heaac_spectral_tools_streams": (I, [P, I, P, P, P, P, P, P, Z, Z, P]),
    "heaac_spectral_tools_streams_ex": (I, [P, I, P, P, P, P, P, P, Z, Z, P, P]),
    "heaac_spectral_tools_batch_ex": (I, [P, I, I, P, P, P, P, P, P, P, P, I, Z, P]),
    "heaac_sbr_make_header": (I, [P, I, I, I, I, I, I, I, I, I, I, I, I]),
    "heaac_build_info": (S, []),
    # heaac_fft.h
    "ff_fft_init": (I, [P, I, I]),
    "ff_fft_end": (None, [P]),
    "ff_fft_permute": (None, [P, P]),
    "ff_fft_calc": (None, [P, P]),
    "ff_mdct_init": (I, [P, I, I, D]),
    "ff_mdct_end": (None, [P]),
    "ff_imdct_half": (None, [P, P, P]),
    "ff_imdct_calc": (None, [P, P, P]),
    "ff_kbd_window_init": (None, [P, F, I]),
    "ff_sine_window_init": (None, [P, I]),
    "ff_init_ff_sine_windows": (None, [I]),
    "av_fft_init": (P, [I, I]),
    "av_fft_permute": (None, [P, P]),
    "av_fft_calc": (None, [P, P]),
    "av_fft_end": (None, [P]),
    "av_mdct_init": (P, [I, I, D]),
    "av_imdct_calc": (None, [P, P, P]),
    "av_imdct_half": (None, [P, P, P]),
    "av_mdct_calc": (None, [P, P, P]),
    "av_mdct_end": (None, [P]),
    # heaac_codec.h
    "heaac_codec_get_context_defaults": (None, [P]),
    "heaac_codec_open": (I, [P, P]),
    "heaac_codec_decode": (I, [P, P, P, P]),
    "heaac_codec_close": (I, [P]),
    # heaac_parse.h
    "heaac_asc_parse": (I, [P, P, I]),
    "heaac_ga_specific_config": (I, [P, P, I, I]),
    "heaac_adts_parse_header": (I, [P, P, I]),
    "heaac_adts_probe": (I, [P, Z]),
    "heaac_adts_split": (C.c_long, [P, Z, P, Z, P]),
    "heaac_aac_parse_frame": (I, [P, P, P, I, P, P, P, P]),
    "heaac_aac_parse_frame_ex": (I, [P, P, P, I, I, P, P, P, P, P]),
    "heaac_aac_layout_default": (I, [P, I]),
    "heaac_aac_layout_from_pce": (I, [P, P, I, I, P]),
    "heaac_aac_layout_from_au": (I, [P, P, I]),
    "heaac_asc_layout": (I, [P, P, P, I]),
    "heaac_aac_parse_frame_layout": (I, [P, P, P, P, I, P, P, P, P, P]),
    "heaac_aac_parse_frame_layout_ex": (I, [P, P, P, P, I, P, P, P, P, P, P]),
    "heaac_aac_parse_batch": (I, [P, P, P, P, Z, P, P, P, P, P, I]),
    "heaac_aac_parse_device": (I, [P, P, P, P, P, Z, I, P, P, P, P, P, P]),
    "heaac_aac_tables_fingerprint": (C.c_uint64, []),
    "heaac_sbr_table_create": (P, [Z]),
    "heaac_sbr_table_destroy": (None, [P]),
    "heaac_sbr_table_count": (Z, [P]),
    "heaac_sbr_table_data": (P, [P]),
    "heaac_sbr_stream_init": (None, [P, Z]),
    "heaac_sbr_stream_bytes": (Z, []),
    "heaac_sbr_parse_payload": (I, [P, P, I, P, I, I, I, I, I, I, P, P, P]),
    "heaac_sbr_no_payload": (None, [P, I, P, P]),
    "heaac_heaac_parse_frame": (I, [P, P, P, P, P, I, P, P, P, P, P, P]),
    "heaac_heaac_parse_frame_ex": (I, [P, P, P, P, P, I, I, P, P, P, P, P, P]),
    "heaac_heaac_parse_batch": (I, [P, P, P, P, P, P, Z, P, P, P, P, P, P, P, I]),
    "heaac_sbr_parse_device": (I, [P, P, P, P, P, P, P, P, Z, P, Z, P, P, P, P]),
    "heaac_heaac_parse_device": (I, [P, P, P, P, P, P, P, Z, I, P, P, P, P, P, Z, P, P, P, P]),
    "heaac_aac_parse_device_streams": (I, [P, P, P, P, P, Z, Z, I, P, P, P, P, P, P, P, P]),
    "heaac_heaac_parse_device_streams": (I, [P, P, P, P, P, P, P, Z, Z, I, P, P, P, P, P, Z, P, P, P, P, P, P]),
    "heaac_sbr_tables_fingerprint": (C.c_uint64, []),
    # heaac_pipeline.h
    "heaac_pipeline_create": (I, [P, P, I, Z, I]),
    "heaac_pipeline_destroy": (None, [P]),
    "heaac_pipeline_submit": (I, [P, P, P, P]),
    "heaac_pipeline_create_streams": (I, [P, P, I, Z, Z, I]),
    "heaac_pipeline_frames_per_tick": (Z, [P]),
    "heaac_pipeline_create_ex": (I, [P, P, I, Z, Z, I, I]),
    "heaac_pipeline_parse_counts": (None, [P, P]),
    "heaac_pipeline_collect": (I, [P, P]),
    "heaac_pipeline_timing": (None, [P, P]),
    "heaac_layout_pipeline_create": (I, [P, P, P, Z, I]),
    "heaac_layout_pipeline_destroy": (None, [P]),
    "heaac_layout_pipeline_submit": (I, [P, P, P, P]),
    "heaac_layout_pipeline_collect": (I, [P, P]),
    "heaac_layout_pipeline_channels": (I, [P]),
    # heaac_debug.h
    "heaac_debug_workspace": (I, [P, P, P, P]),
    "heaac_debug_xbands": (I, [P, P, Z]),
    "heaac_debug_aac_parse_core": (I, [P, P, P, P, Z, I, P, P, P, P, P, P]),
    "heaac_debug_sbr_parse_core": (I, [P, P, P, P, P, P, P, Z, P, Z, P, P, P, P]),
    "heaac_debug_aac_parse_core_streams": (I, [P, P, P, P, Z, Z, I, P, P, P, P, P, P, P, P]),
    "heaac_debug_heaac_parse_core_streams": (I, [P, P, P, P, P, P, Z, Z, I, P, P, P, P, P, Z, P, P, P, P, P, P]),
    "heaac_debug_pipeline_pack": (I, [P, P, Z, P, P]),
    "heaac_debug_pipeline_stops": (Z, [P, Z, Z, P, P]),
    # heaac_multi.h
    "heaac_multi_shard": (None, [Z, I, I, P, P]),
    "heaac_multi_create": (I, [P, P, I, Z]),
    "heaac_multi_destroy": (None, [P]),
    "heaac_multi_devices": (I, [P]),
    "heaac_multi_device": (P, [P, I]),
    "heaac_multi_stream": (P, [P, I]),
    "heaac_multi_he_decode": (I, [P, I, I, P, I, P, I]),
}

# Exported, but declared in no header under include/ (the data symbols heaac_aac_decoder and ff_sine_windows have no
# prototype at all).
UNDECLARED = {
    # csrc/tables.h; the name stays c_char_p, as it always was here, where every header prototype takes c_void_p for a
    # pointer: both accept the bytes get_table() passes
    "heaac_get_table": (I, [S, P, I]),
    "heaac_debug_timeline": (I, [P]),                    # csrc/k_ps.hip, builds with -DHEAAC_STAMPS only
    "heaac_debug_timeline_he": (I, [P]),                 # csrc/k_he.hip, likewise
}


def apply(lib):
    """Set restype and argtypes of every function above on `lib`.  One that a header declares must be there (an
    AttributeError otherwise); one without a header only where this build has it."""
    for name, (restype, argtypes) in {**PROTOTYPES, **UNDECLARED}.items():
        if name in PROTOTYPES or hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = restype, argtypes
