// ofdm_phasor.h -- the carrier-offset phasor shared by the packet transmitter (ofdm_transmit.hip) and the channel
// (ofdm_channel.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ofdm {

constexpr double CARRIER_TS = 25e-9;         // sample period of the oversampled waveform (OFDM.c:16-17, x2)

// exp(j 2 pi f m Ts): revolutions in fp64, reduced to [-1/2, 1/2], then the fp32 sine and cosine.  A pure function of
// the sample index m (exact in a double up to 2^53).
__device__ __forceinline__ float2 carrier_phasor(double f, double m) {
    float2 e;
    const double rev = f * m * CARRIER_TS;
    const float r = (float)(rev - rint(rev));
    sincospif(2.0f * r, &e.y, &e.x);
    return e;
}

}  // namespace ofdm
