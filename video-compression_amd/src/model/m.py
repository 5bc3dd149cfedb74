"""``src.model.m`` -- same import path as ICIP2024/src/model/m.py AND ICIP2023/src/model/m.py (the two reference projects share
it): ``FlowGuidedB`` and ``DeformB`` run on MI355X through libvc_hip.so."""
from vcamd.icip2023 import DeformB  # noqa: F401
from vcamd.icip2024 import FlowGuidedB  # noqa: F401
