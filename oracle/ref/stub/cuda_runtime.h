// TEST INFRASTRUCTURE ONLY.  Deliberately empty: the reference's src/sceneStructs.h includes
// <cuda_runtime.h>, which a host-only compile of its headers (oracle/ref/Makefile, target ref_bounce)
// neither has nor needs -- hipcc supplies __host__ / __device__.
#pragma once
