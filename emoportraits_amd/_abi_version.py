EMO_ABI_VERSION = 26   # must equal EMO_ABI_VERSION in include/emo_hip.h
