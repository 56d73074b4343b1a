EMO_ABI_VERSION = 23   # must equal EMO_ABI_VERSION in include/emo_hip.h
