EMO_ABI_VERSION = 14   # must equal EMO_ABI_VERSION in include/emo_hip.h
