function M = shRotationMatrix(order, yawRad, pitchRad, rollRad, shDefinition)
% The SH rotation matrix of rotateSH, [(N+1)^2 x (N+1)^2] for order N <= 15: rotateSH(x, yaw, pitch, roll) == x * M.'.
% Block-diagonal by order, orthogonal ('real') or unitary ('complex').  Takes angles in radians; polarch's getSHrotMtx takes a
% 3 x 3 rotation matrix instead.
if nargin < 5; shDefinition = 'real'; end
M = emagls_mex('shrotmtx', double(order), double(yawRad), double(pitchRad), double(rollRad), shDefinition);
end
