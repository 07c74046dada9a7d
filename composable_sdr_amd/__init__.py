"""MI355X-native DSP chain behind ComposableSDR's Pipe API.

Thin ctypes binding over libcsdr_hip.so (C ABI in include/csdr.h; hand-written HIP
kernels for gfx950).  There is no CPU fallback: importing works without a GPU (so the
symbol table can be checked), but creating any object without one raises CsdrError.
"""
from ._lib import CsdrError, lib, lib_path, build_library, DEMOD_NONE, DEMOD_FM, DEMOD_AM, DEMOD_WBFM  # noqa: F401
from .pipes import (  # noqa: F401
    Pipe, compose, Chain, ChainConfig, dcBlocker, mixDown, mixUp, automaticGainControl,
    fmDemodulator, amDemodulator, resampler, iirFilter, firDecimator, wbFMDemodulator, firpfbchChannelizer,
    FmStereo, stereoFMDecoder, SymSync, symSyncR, fmDemWithSync, FirHilb, realToComplex, complexToReal,
    symSyncC, firdes_rnyquist, CSDR_FIRFILT_ARKAISER, CSDR_FIRFILT_RRC,
    FskDem, fskDemodulator, FirFilt, firFilterCKaiser, firFilterC, firFilterR, firdes_kaiser, fir_groupdelay,
    IirSos, iirCFilter, iirFilterN, iirFilterSOS, iirdes_butter_lowpass,
    GmskDem, gmskDemodulator, firdes_gmsktx, firdes_gmskrx, firFilterRNyquist,
    Firpfbch2, firpfbch2Channelizer, firdes_pfbch2,
    Firpfbch2Synth, firpfbch2Synthesizer, firdes_pfbsyn2,
    RowResamp, rowResampler, firdes_rowresamp,
    PskTrack, pskTracker, SymTrack, symTracker, sincos_word, CSDR_PSKTRACK_EQ_DD, CSDR_PSKTRACK_EQ_CM,
)
from .trans import compact, takeNArr, mix, mux, distribute_, addPipe  # noqa: F401
