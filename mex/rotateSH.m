function out = rotateSH(in, yawRad, pitchRad, rollRad, shDefinition)
% Three-axis rotation of an SH signal [numSamples x (N+1)^2] (ACN, N <= 15) on the GPU: rotateHOA_N3D(in, yaw, pitch, roll) with
% angles in radians, own specification (DESIGN.md section 7).  R = Rz(yaw) * Ry(pitch) * Rx(roll) with getSH's axes (x front,
% y left, z up); the signal of a plane wave from u, conj(getSH(N, u, shDefinition)), becomes the one from R * u.  Each angle is a
% scalar or one angle per sample.  shDefinition: 'real' (default) or 'complex'.
if nargin < 5; shDefinition = 'real'; end
out = emagls_mex('rotate3', double(in), double(yawRad), double(pitchRad), double(rollRad), shDefinition);
end
