EMO_ABI_VERSION = 13   # must equal EMO_ABI_VERSION in include/emo_hip.h
